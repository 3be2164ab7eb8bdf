"""CPU yardstick of ``dsm_mobile_records`` and ``dsm_normal_records`` in plain Python, written from the text of include/diffspectra_mobile.h
and not from the kernel: the fold, the charge normalisation, donors, acceptors and interior atoms, the shift paths by brute-force
enumeration of every simple path (``simple_paths``: it tries every neighbour and tests the bond orders and the atoms as rule 4 states them,
without the shortcut that an interior atom has one double bond), the groups by union-find, the search of rule 6 for the node count, and the
normal form byte for byte.  It works on raw record bytes, so whatever the contract says is ignored can hold garbage.  Identity of normal
forms is ``graph_mirror.same_graph``.

Also here: the hand-stated table of molecules with their donors, acceptors, groups, hydrogens and proton balance and the hand-stated pairs
with their verdict and layer (the pin: InChI cannot run where the project runs), ``shifted`` (one hydrogen moved along one path) and the
seeded corpus of random closed-shell molecules that the CPU test checks for coverage and the GPU test compares on.
"""
from __future__ import annotations

import numpy as np

from tests import graph_mirror as GM, groups_mirror as G, structure_mirror as SM, valence_mirror as VM

OK, UNDECIDED, UNUSABLE, OVERFLOW = 0, 2, 3, 4
W = SM.W
MAX_NODES, MAX_GROUPS, GROUP_TYPE, PROTON_TYPE, DEFAULT_NODES = 1 << 20, 14, 6, 7, 4096
H, C, N, O, F = range(5)
KEYS = ("fixed_h", "q_res", "group_of", "group_h", "summary", "nodes", "status")
NORMAL_KEYS = ("out_rec", "out_n", "out_source", "status")
DIFFERENT, IDENTICAL, PAIR_UNDECIDED, INVALID = 0, 1, 2, 3


class Analysis:
    """One record as the header sees it.  ``kept`` [atoms], ``ht`` / ``q_res`` {kept atom: value} after rule 2, ``p``, ``donors``, ``acceptors``,
    ``interior``, ``paths`` (every simple shift path, as atom tuples), ``groups`` [sorted members] by lowest atom, ``nodes`` of rule 6."""

    def __init__(self, rec, n, max_nodes=DEFAULT_NODES):
        self.n, self.types, self.raw, self.orders, self.usable, _ = VM.read(rec, n, VM.RECORD)
        self.status = OK if self.usable else UNUSABLE
        if not self.usable:
            return
        n, t, raw, order = self.n, self.types, self.raw, self.orders
        nbrs = [[j for j in range(n) if order[i][j]] for i in range(n)]
        folded = {i for i in range(n) if t[i] == H and raw[i] == 0 and len(nbrs[i]) == 1 and order[i][nbrs[i][0]] == 1 and t[nbrs[i][0]] != H}
        self.kept = [i for i in range(n) if i not in folded]
        q = {i: VM.applied_charge(t[i], raw[i]) for i in self.kept}
        self.dbl = {i: sum(order[i][j] == 2 for j in nbrs[i]) for i in self.kept}
        trp = {i: sum(order[i][j] == 3 for j in nbrs[i]) for i in self.kept}
        self.ht = {i: sum(j in folded for j in nbrs[i]) + max(0, VM.VMAX[t[i], q[i]] - sum(order[i])) for i in self.kept}
        self.nbrs = {i: [j for j in nbrs[i] if j not in folded] for i in self.kept}
        # rule 2, judged on the input
        self.q_res, self.p = dict(q), 0
        for i in self.kept:
            if q[i] and any(q[j] * q[i] < 0 for j in self.nbrs[i]):
                continue
            if t[i] == N and q[i] == 1 and self.ht[i] >= 1:
                self.ht[i], self.q_res[i], self.p = self.ht[i] - 1, 0, self.p + 1
            elif t[i] in (N, O) and q[i] == -1:
                self.ht[i], self.q_res[i], self.p = self.ht[i] + 1, 0, self.p - 1
        candidate = [i for i in self.kept if t[i] in (N, O) and self.q_res[i] == 0 and trp[i] == 0 and self.dbl[i] <= 1]
        self.donors = [i for i in candidate if self.ht[i] >= 1 and self.dbl[i] == 0]
        self.acceptors = [i for i in candidate if self.dbl[i] == 1]
        self.interior = {i for i in self.kept if t[i] in (C, N) and self.q_res[i] == 0 and self.dbl[i] == 1 and trp[i] == 0}
        self.paths = [path for d in self.donors for path in self.simple_paths(d)]
        self.nodes = sum(self.search(d, max_nodes)[1] for d in self.donors) if self.acceptors else 0
        if self.nodes > max_nodes:
            self.status = UNDECIDED
            return
        parent = {i: i for i in self.kept}

        def find(a):
            while parent[a] != a:
                a = parent[a]
            return a
        for path in self.paths:
            a, b = find(path[0]), find(path[-1])
            parent[max(a, b)] = min(a, b)
        members = {}
        for i in self.kept:
            members.setdefault(find(i), []).append(i)
        self.groups = [sorted(m) for root, m in sorted(members.items()) if len(m) > 1]
        self.group_of = {i: g for g, m in enumerate(self.groups) for i in m}
        self.group_h = [sum(self.ht[i] for i in m) for m in self.groups]
        self.fixed = {i: 0 if i in self.group_of else self.ht[i] for i in self.kept}

    def simple_paths(self, donor):
        """Every simple path of rule 4 from ``donor``, by trying every neighbour: bond k of the path has order 1 (k even) or 2 (k odd), the
        atoms between the ends are interior atoms, an even position on an acceptor is a path."""
        out = []

        def walk(path):
            k = len(path) - 1                                                    # bonds so far
            for v in self.nbrs[path[-1]]:
                if v in path or self.orders[path[-1]][v] != (1 if k % 2 == 0 else 2):
                    continue
                if k % 2 == 1 and v in self.acceptors:
                    out.append(tuple(path) + (v,))
                if v in self.interior:
                    walk(path + [v])
        walk([donor])
        return out

    def walk_reaches(self, donor):
        """The acceptors an alternating WALK from ``donor`` reaches (atoms may repeat): what rule 4 must not be."""
        seen, todo, out = {(donor, 0)}, [(donor, 0)], set()
        while todo:
            u, k = todo.pop()
            for v in self.nbrs[u]:
                if self.orders[u][v] != (1 if k == 0 else 2):
                    continue
                if k == 1 and v in self.acceptors:
                    out.add(v)
                if v in self.interior and (v, 1 - k) not in seen:
                    seen.add((v, 1 - k))
                    todo.append((v, 1 - k))
        return out

    def search(self, donor, max_nodes):
        """Rule 6 for one donor: (acceptors found, nodes; counting stops at max_nodes + 1)."""
        found, count, accept = set(), [0], set(self.acceptors)

        class Done(Exception):
            pass

        def extend(u, onpath):
            for v in self.nbrs[u]:                                               # ascending
                if self.orders[u][v] != 1 or v not in self.interior or v in onpath:
                    continue
                count[0] += 1
                if count[0] > max_nodes:
                    raise Done
                w = [j for j in self.nbrs[v] if self.orders[v][j] == 2][0]
                if w in onpath:
                    continue
                if w in accept:
                    found.add(w)
                    if found == accept:
                        raise Done
                if w in self.interior:
                    extend(w, onpath | {v, w})
        try:
            extend(donor, {donor})
        except Done:
            pass
        return found, count[0]


def analyse(rec, n, max_nodes=DEFAULT_NODES, found=None):
    """One row of ``dsm_mobile_records`` as a dict of KEYS."""
    A = Analysis(rec, n, max_nodes) if found is None else found
    if A.status != OK:
        return dict(fixed_h=[0xff] * W, q_res=[0] * W, group_of=[0xff] * W, group_h=[0xff] * MAX_GROUPS, summary=(0, 0, 0, 0), nodes=0, status=A.status)
    return dict(fixed_h=[A.fixed.get(i, 0xff) for i in range(W)], q_res=[A.q_res.get(i, 0) for i in range(W)],
                group_of=[A.group_of.get(i, 0xff) for i in range(W)], group_h=A.group_h + [0xff] * (MAX_GROUPS - len(A.group_h)),
                summary=(len(A.kept), len(A.groups), sum(A.group_h), A.p), nodes=A.nodes, status=OK)


def analyse_table(rec, n, max_nodes=DEFAULT_NODES):
    return [analyse(r, k, max_nodes) for r, k in zip(np.asarray(rec), np.asarray(n))]


def as_arrays(rows):
    """The rows of ``analyse_table`` as the seven arrays of the kernel."""
    P = len(rows)
    col = lambda key, dtype, *shape: np.array([r[key] for r in rows], dtype).reshape(P, *shape)
    return (col("fixed_h", np.uint8, W), col("q_res", np.int8, W), col("group_of", np.uint8, W), col("group_h", np.uint8, MAX_GROUPS),
            col("summary", np.int32, 4), col("nodes", np.int32), col("status", np.uint8))


def normal_row(rec, n, max_nodes=DEFAULT_NODES, found=None):
    """One row of ``dsm_normal_records``: (record bytes uint8 [1248], out_n, source [29], status)."""
    A = Analysis(rec, n, max_nodes) if found is None else found
    out, source = np.zeros(SM.RECORD_BYTES, np.uint8), [0xff] * W
    if A.status != OK:
        return out, 0, source, A.status
    K = len(A.kept)
    total = K + len(A.groups) + (A.p != 0)
    if total > W:
        return out, 0, source, OVERFLOW
    rec = np.ascontiguousarray(np.asarray(rec, np.uint8))
    pos_in = rec[SM.POS:SM.TYPE].reshape(W, 12)
    pos, bond = out[SM.POS:SM.TYPE].reshape(W, 12), out[SM.BOND:SM.BOND_END].reshape(W, W)
    slot = {a: r for r, a in enumerate(A.kept)}
    for a, r in slot.items():
        pos[r] = pos_in[a]
        out[SM.TYPE + r], out[SM.FC + r], source[r] = A.types[a], A.fixed[a] + 16 * (A.q_res[a] + 1), a
        for b in A.nbrs[a]:
            bond[r, slot[b]] = 1
    for g, members in enumerate(A.groups):
        out[SM.TYPE + K + g], out[SM.FC + K + g] = GROUP_TYPE, A.group_h[g]
        for a in members:
            bond[slot[a], K + g] = bond[K + g, slot[a]] = 1
    if A.p:
        out[SM.TYPE + total - 1], out[SM.FC + total - 1] = PROTON_TYPE, A.p & 255
    return out, total, source, OK


def normal_table(rec, n, max_nodes=DEFAULT_NODES):
    """(out_rec [P, 1248], out_n [P], out_source [P, 29], status [P]) of a record table."""
    rows = [normal_row(r, k, max_nodes) for r, k in zip(np.asarray(rec), np.asarray(n))]
    P = len(rows)
    return (np.stack([r[0] for r in rows]) if P else np.zeros((0, SM.RECORD_BYTES), np.uint8), np.array([r[1] for r in rows], np.int32),
            np.array([r[2] for r in rows], np.uint8).reshape(P, W), np.array([r[3] for r in rows], np.uint8))


def normal_mol(mol, max_nodes=DEFAULT_NODES):
    """(normal form of a molecule dict as a molecule dict, source, status)."""
    rec, n = SM.records([mol])
    out, m, source, status = normal_row(rec[0], n[0], max_nodes)
    return SM.mol_from_record(out, m), source, status


def identity(a, b, max_nodes=DEFAULT_NODES):
    """(verdict, strict verdict, layer, map) of ``mobile_identity_batch`` for the probe ``a`` and the ground truth ``b``: the map sends the
    original kept atoms of ``a`` to those of ``b``, -1 elsewhere."""
    strict = IDENTICAL if GM.same_graph(a, b) else DIFFERENT
    (na, sa, ta), (nb, sb, tb) = normal_mol(a, max_nodes), normal_mol(b, max_nodes)
    if UNUSABLE in (ta, tb):
        return INVALID, strict, -1, None
    if ta != OK or tb != OK:
        return PAIR_UNDECIDED, strict, -1, None
    same, image = GM.same_graph(na, nb, want_map=True)
    if not same:
        return DIFFERENT, strict, -1, None
    return IDENTICAL, strict, 0 if strict == IDENTICAL else 1, image


def classes(mols, max_nodes=DEFAULT_NODES):
    """``mobile_classes``: for every molecule the lowest index of a molecule with the same normal form (every status OK)."""
    forms, out = [normal_mol(m, max_nodes)[0] for m in mols], []
    for i, f in enumerate(forms):
        out.append(next(j for j in range(i + 1) if GM.same_graph(forms[j], f)))
    return out


# ------------------------------------------------------------------------------------------------------------------ molecules

def renumbered(mol, perm):
    """New atom i is old atom perm[i]."""
    perm = np.asarray(perm)
    return dict(pos=np.asarray(mol["pos"])[perm], type=np.asarray(mol["type"])[perm].copy(), fc=np.asarray(mol["fc"])[perm].copy(),
                bond=np.asarray(mol["bond"])[np.ix_(perm, perm)].copy())


def moved(values, perm, fill):
    """A per-atom list of W entries after ``renumbered(mol, perm)``."""
    return [values[int(old)] for old in perm] + [fill] * (W - len(perm))


def shifted(mol, path):
    """``mol`` with one explicit hydrogen of the donor ``path[0]`` moved to the acceptor ``path[-1]`` and the bond orders along ``path``
    exchanged (1 <-> 2): the other tautomer, atoms numbered alike.  None when the donor has no explicit plain hydrogen to give."""
    types, bond = np.asarray(mol["type"]), np.asarray(mol["bond"]).copy()
    d, a = path[0], path[-1]
    hs = [h for h in range(len(types)) if types[h] == H and mol["fc"][h] == 0 and bond[d, h] == 1 and (bond[h] > 0).sum() == 1]
    if not hs:
        return None
    h = hs[0]
    bond[d, h] = bond[h, d] = 0
    bond[a, h] = bond[h, a] = 1
    for u, v in zip(path, path[1:]):
        bond[u, v] = bond[v, u] = 3 - bond[u, v]
    return dict(pos=np.asarray(mol["pos"]).copy(), type=types.copy(), fc=np.asarray(mol["fc"]).copy(), bond=bond)


def _benzene(first_double=True):
    return G._ring(first_double)


def hand_table():
    """[(name, molecule, stated)] with stated = dict(donors, acceptors, groups, group_h, fixed_h [per heavy atom], p, q_res [per heavy atom]):
    stated by hand from the header's rules, not computed.  The heavy atoms come first in every molecule (G.molecule appends the hydrogens),
    and every heavy atom is a kept atom."""
    mol = G.molecule

    def row(name, elements, bonds, hydrogens, donors=(), acceptors=(), groups=(), group_h=(), fixed_h=None, p=0, fc=None, q_res=None):
        k = len(elements)
        return (name, mol(elements, bonds, hydrogens, fc),
                dict(donors=list(donors), acceptors=list(acceptors), groups=[list(g) for g in groups], group_h=list(group_h),
                     fixed_h=list(hydrogens) if fixed_h is None else list(fixed_h), p=p, q_res=[0] * k if q_res is None else list(q_res)))
    a, b = _benzene(True), _benzene(False)
    return [
        # N1(H) C2 N3 C4(CH3) C5: the path 0-1=2
        row("4-methylimidazole", "NCNCCC", [(0, 1, 1), (1, 2, 2), (2, 3, 1), (3, 4, 2), (4, 0, 1), (3, 5, 1)], [1, 1, 0, 0, 1, 3],
            [0], [2], [(0, 2)], [1], [0, 1, 0, 0, 1, 3]),
        row("5-methylimidazole", "NCNCCC", [(0, 1, 2), (1, 2, 1), (2, 3, 1), (3, 4, 2), (4, 0, 1), (3, 5, 1)], [0, 1, 1, 0, 1, 3],
            [2], [0], [(0, 2)], [1], [0, 1, 0, 0, 1, 3]),
        # N1(H) N2 C3(CH3) C4 C5: 0-1 is a single bond into N2, whose double bond leads away; the path is 0-4=3-2=1, four bonds
        row("3-methylpyrazole", "NNCCCC", [(0, 1, 1), (1, 2, 2), (2, 3, 1), (3, 4, 2), (4, 0, 1), (2, 5, 1)], [1, 0, 0, 1, 1, 3],
            [0], [1], [(0, 1)], [1], [0, 0, 0, 1, 1, 3]),
        row("5-methylpyrazole", "NNCCCC", [(0, 1, 1), (1, 2, 1), (2, 3, 2), (3, 4, 1), (4, 0, 2), (2, 5, 1)], [0, 1, 0, 1, 1, 3],
            [1], [0], [(0, 1)], [1], [0, 0, 0, 1, 1, 3]),
        row("acetamide", "CCON", [(0, 1, 1), (1, 2, 2), (1, 3, 1)], [3, 0, 0, 2], [3], [2], [(2, 3)], [2], [3, 0, 0, 0]),
        row("acetimidic acid", "CCON", [(0, 1, 1), (1, 2, 1), (1, 3, 2)], [3, 0, 1, 1], [2], [3], [(2, 3)], [2], [3, 0, 0, 0]),
        # N0 C1(O6) C2 C3 C4 C5: the paths 0-1=6 and 0-5=4-3=2-1=6 in one drawing
        row("2-pyridone", "NCCCCCO", [(0, 1, 1), (1, 6, 2), (1, 2, 1), (2, 3, 2), (3, 4, 1), (4, 5, 2), (5, 0, 1)], [1, 0, 1, 1, 1, 1, 0],
            [0], [6], [(0, 6)], [1], [0, 0, 1, 1, 1, 1, 0]),
        row("2-hydroxypyridine, N=C(OH)", "NCCCCCO", a + [(1, 6, 1)], [0, 0, 1, 1, 1, 1, 1], [6], [0], [(0, 6)], [1], [0, 0, 1, 1, 1, 1, 0]),
        row("2-hydroxypyridine, N-C(OH)", "NCCCCCO", b + [(1, 6, 1)], [0, 0, 1, 1, 1, 1, 1], [6], [0], [(0, 6)], [1], [0, 0, 1, 1, 1, 1, 0]),
        row("4-pyridone", "NCCCCCO", [(0, 1, 1), (1, 2, 2), (2, 3, 1), (3, 6, 2), (3, 4, 1), (4, 5, 2), (5, 0, 1)], [1, 1, 1, 0, 1, 1, 0],
            [0], [6], [(0, 6)], [1], [0, 1, 1, 0, 1, 1, 0]),
        row("4-hydroxypyridine", "NCCCCCO", a + [(3, 6, 1)], [0, 1, 1, 0, 1, 1, 1], [6], [0], [(0, 6)], [1], [0, 1, 1, 0, 1, 1, 0]),
        row("acetic acid", "CCOO", [(0, 1, 1), (1, 2, 2), (1, 3, 1)], [3, 0, 0, 1], [3], [2], [(2, 3)], [1], [3, 0, 0, 0]),
        row("acetic acid, the other oxygen", "CCOO", [(0, 1, 1), (1, 2, 1), (1, 3, 2)], [3, 0, 1, 0], [2], [3], [(2, 3)], [1], [3, 0, 0, 0]),
        # the amine is a donor, but its carbon has no double bond: no path from it
        row("glycine", "NCCOO", [(0, 1, 1), (1, 2, 1), (2, 3, 2), (2, 4, 1)], [2, 2, 0, 0, 1], [0, 4], [3], [(3, 4)], [1], [2, 2, 0, 0, 0]),
        row("glycine zwitterion", "NCCOO", [(0, 1, 1), (1, 2, 1), (2, 3, 2), (2, 4, 1)], [3, 2, 0, 0, 0], [0, 4], [3], [(3, 4)], [1], [2, 2, 0, 0, 0],
            fc=[1, 0, 0, 0, -1]),
        row("ammonium", "N", [], [4], [0], fixed_h=[3], p=1, fc=[1]),
        row("ammonia", "N", [], [3], [0]),
        # both charges are paired and stay; the oxygen is no candidate
        row("pyridine N-oxide", "NCCCCCO", a + [(0, 6, 1)], [0, 1, 1, 1, 1, 1, 0], fc=[1, 0, 0, 0, 0, 0, -1], q_res=[1, 0, 0, 0, 0, 0, -1]),
        row("nitromethane", "CNOO", [(0, 1, 1), (1, 2, 2), (1, 3, 1)], [3, 0, 0, 0], [], [2], fc=[0, 1, 0, -1], q_res=[0, 1, 0, -1]),
        row("acetate", "CCOO", [(0, 1, 1), (1, 2, 2), (1, 3, 1)], [3, 0, 0, 0], [3], [2], [(2, 3)], [1], [3, 0, 0, 0], p=-1, fc=[0, 0, 0, -1]),
        row("pyridinium", "NCCCCC", a, [1, 1, 1, 1, 1, 1], [], [0], fixed_h=[0, 1, 1, 1, 1, 1], p=1, fc=[1, 0, 0, 0, 0, 0]),
        row("pyridine", "NCCCCC", a, [0, 1, 1, 1, 1, 1], [], [0]),
        row("tetramethylammonium", "NCCCC", [(0, 1, 1), (0, 2, 1), (0, 3, 1), (0, 4, 1)], [0, 3, 3, 3, 3], fc=[1, 0, 0, 0, 0], q_res=[1, 0, 0, 0, 0]),
        row("acetone", "CCCO", [(0, 1, 1), (1, 2, 1), (1, 3, 2)], [3, 0, 3, 0], [], [3]),
        row("propen-2-ol", "CCCO", [(0, 1, 2), (1, 2, 1), (1, 3, 1)], [2, 0, 3, 1], [3], []),
        row("p-aminophenol", "CCCCCCNO", a + [(0, 6, 1), (3, 7, 1)], [0, 1, 1, 0, 1, 1, 2, 1], [6, 7], []),
        # HO-C1(=C2)-CH=O with C2 in a cyclopropene C2 C3=C4: the walk 0-1=2-3=4-2=1-5=6 comes back to atom 1 through the odd ring and leaves
        # it for the aldehyde; a simple path cannot, because the double bond of atom 1 leads into the ring
        row("2-(cycloprop-2-en-1-ylidene)-2-hydroxyacetaldehyde", "OCCCCCO", [(0, 1, 1), (1, 2, 2), (2, 3, 1), (3, 4, 2), (4, 2, 1), (1, 5, 1), (5, 6, 2)],
            [1, 0, 0, 1, 1, 1, 0], [0], [6]),
        # both amines reach the imine: one group of three by merging
        row("guanidine", "CNNN", [(0, 1, 2), (0, 2, 1), (0, 3, 1)], [0, 1, 2, 2], [2, 3], [1], [(1, 2, 3)], [5], [0, 0, 0, 0]),
        row("guanidine, the other nitrogen", "CNNN", [(0, 1, 1), (0, 2, 2), (0, 3, 1)], [0, 2, 1, 2], [1, 3], [2], [(1, 2, 3)], [5], [0, 0, 0, 0]),
        # the nitrogen is an acceptor and an interior atom: 3-4=... the path from N-H reaches both oxygens, and in the iminol the path
        # 2-1=3-4=5 runs through the nitrogen
        row("diacetamide", "CCONCOC", [(0, 1, 1), (1, 2, 2), (1, 3, 1), (3, 4, 1), (4, 5, 2), (4, 6, 1)], [3, 0, 0, 1, 0, 0, 3],
            [3], [2, 5], [(2, 3, 5)], [1], [3, 0, 0, 0, 0, 0, 3]),
        row("diacetamide, an iminol", "CCONCOC", [(0, 1, 1), (1, 2, 1), (1, 3, 2), (3, 4, 1), (4, 5, 2), (4, 6, 1)], [3, 0, 1, 0, 0, 0, 3],
            [2], [3, 5], [(2, 3, 5)], [1], [3, 0, 0, 0, 0, 0, 3]),
        row("o-xylene, C1=C2", "CCCCCCCC", a + [(0, 6, 1), (1, 7, 1)], [0, 0, 1, 1, 1, 1, 3, 3]),
        row("o-xylene, C1-C2", "CCCCCCCC", b + [(0, 6, 1), (1, 7, 1)], [0, 0, 1, 1, 1, 1, 3, 3]),
        row("propan-1-ol", "CCCO", [(0, 1, 1), (1, 2, 1), (2, 3, 1)], [3, 2, 2, 1], [3], []),
        row("propan-2-ol", "CCCO", [(0, 1, 1), (1, 2, 1), (1, 3, 1)], [3, 1, 3, 1], [3], []),
        row("ethanol", "CCO", [(0, 1, 1), (1, 2, 1)], [3, 2, 1], [2], []),
        row("dimethyl ether", "COC", [(0, 1, 1), (1, 2, 1)], [3, 0, 3]),
    ]


def named(name):
    return [mol for nm, mol, _ in hand_table() if nm == name][0]


def hand_pairs():
    """[(name of a, name of b, verdict, layer)], stated by hand: layer 0 = the same graph as drawn, 1 = the same only in the normal form, -1 =
    not the same."""
    same, differ = (IDENTICAL, 1), (DIFFERENT, -1)
    return [
        ("4-methylimidazole", "5-methylimidazole", *same),
        ("3-methylpyrazole", "5-methylpyrazole", *same),
        ("acetamide", "acetimidic acid", *same),
        ("2-pyridone", "2-hydroxypyridine, N=C(OH)", *same),
        ("2-pyridone", "2-hydroxypyridine, N-C(OH)", *same),
        ("2-hydroxypyridine, N=C(OH)", "2-hydroxypyridine, N-C(OH)", *same),
        ("4-pyridone", "4-hydroxypyridine", *same),
        ("acetic acid", "acetic acid, the other oxygen", IDENTICAL, 0),      # the two drawings are one labelled graph: the oxygens change places
        ("glycine", "glycine zwitterion", *same),
        ("guanidine", "guanidine, the other nitrogen", IDENTICAL, 0),
        ("diacetamide", "diacetamide, an iminol", *same),
        ("o-xylene, C1=C2", "o-xylene, C1-C2", *same),
        ("4-methylimidazole", "4-methylimidazole", IDENTICAL, 0),
        ("acetone", "propen-2-ol", *differ),
        ("propan-1-ol", "propan-2-ol", *differ),
        ("ethanol", "dimethyl ether", *differ),
        ("ammonium", "ammonia", *differ),
        ("pyridinium", "pyridine", *differ),
        ("acetate", "acetic acid", *differ),
        ("4-pyridone", "2-pyridone", *differ),
        ("acetamide", "acetic acid", *differ),
        ("3-methylpyrazole", "4-methylimidazole", *differ),
        ("2-hydroxypyridine, N=C(OH)", "4-hydroxypyridine", *differ),
        ("nitromethane", "acetate", *differ),
    ]


# ------------------------------------------------------------------------------------------------------------------ the corpus

_CAP = {C: 4, N: 3, O: 2, F: 1}


def random_closed_shell(rng, heavy, core=False):
    """A random closed-shell molecule of ``heavy`` C / N / O / F atoms with explicit hydrogens: a random tree, up to two ring closures that
    make rings of 3 to 6, bond orders raised where both ends have room, now and then an ammonium / oxide pair of charges, hydrogens to fill.
    ``core``: the first atoms are a chain X-c=c-...-c=Y of 3, 5 or 7 atoms with X and Y among N and O and the atoms between among C and N, which
    the rest of the tree grows on."""
    while True:
        types = [int(t) for t in rng.choice([C, N, O, F], size=heavy, p=[0.5, 0.25, 0.2, 0.05])]
        order = np.zeros((heavy, heavy), np.int64)
        chain = 0
        if core:
            chain = min(int(rng.choice([3, 5, 7], p=[0.45, 0.35, 0.2])), heavy if heavy % 2 else heavy - 1)
            types[:chain] = [int(rng.choice([N, O]))] + [int(rng.choice([C, N], p=[0.85, 0.15])) for _ in range(chain - 2)] + [int(rng.choice([N, O]))]
            for i in range(chain - 1):
                order[i, i + 1] = order[i + 1, i] = 1 + i % 2
        room = [_CAP[t] - int(order[i].sum()) for i, t in enumerate(types)]
        ok = chain <= heavy and min(room) >= 0
        for i in range(max(chain, 1), heavy):
            free = [j for j in range(i) if room[j] > 0]
            if not ok or not free or room[i] == 0:
                ok = False
                break
            j = int(rng.choice(free))
            order[i, j] = order[j, i] = 1
            room[i] -= 1
            room[j] -= 1
        if ok:
            break

    def distance(a, b):
        seen, todo = {a: 0}, [a]
        while todo:
            u = todo.pop(0)
            for v in np.nonzero(order[u])[0]:
                if int(v) not in seen:
                    seen[int(v)] = seen[u] + 1
                    todo.append(int(v))
        return seen.get(b, 99)
    for _ in range(int(rng.integers(3))):
        pairs = [(i, j) for i in range(heavy) for j in range(i + 1, heavy) if room[i] and room[j] and not order[i, j] and 2 <= distance(i, j) <= 5]
        if pairs:
            i, j = pairs[int(rng.integers(len(pairs)))]
            order[i, j] = order[j, i] = 1
            room[i] -= 1
            room[j] -= 1
    for _ in range(int(rng.integers(0, 3) if core else rng.integers(1, 6))):
        bonds = [(i, j) for i in range(heavy) for j in range(i + 1, heavy) if order[i, j] and order[i, j] < 3 and room[i] and room[j]]
        if bonds:
            i, j = bonds[int(rng.integers(len(bonds)))]
            order[i, j] += 1
            order[j, i] += 1
            room[i] -= 1
            room[j] -= 1
    fc = [0] * heavy
    if rng.random() < 0.4:
        plus = [i for i in range(heavy) if types[i] == N]
        minus = [i for i in range(heavy) if types[i] == O and room[i] == 1]
        if plus and minus:
            i, j = int(rng.choice(plus)), int(rng.choice(minus))
            fc[i], fc[j] = 1, -1
            room[i] += 1
            room[j] -= 1
    bonds = [(i, j, int(order[i, j])) for i in range(heavy) for j in range(i + 1, heavy) if order[i, j]]
    return G.molecule("".join("HCNOF"[t] for t in types), bonds, room, fc)


def corpus(seed=20261021, count=240):
    """The seeded corpus: ``count`` molecules of 2 to 9 heavy atoms, each of at most 29 atoms; two in three grow on a conjugated chain between
    two N / O atoms, the others on nothing."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        core = len(out) % 3 != 0
        mol = random_closed_shell(rng, int(rng.integers(3 if core else 2, 10)), core)
        if len(mol["type"]) <= W:
            out.append(mol)
    return out
