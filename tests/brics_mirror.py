"""CPU yardstick of ``dsb_brics_records`` and ``dsb_brics_fragment_records`` and of the Frag arithmetic in plain Python, written from the text of
include/diffspectra_brics.h and not from the kernel: the thirteen environments as searches over distinct neighbours, the rule walk, the
fragments by a depth-first search without the cuts, and the fragment records byte for byte.  The graph perception (the fold, ring bonds,
aromatic cycles, the eight bond classes) is that of tests/substructure_mirror.py, as the header refers to diffspectra_substructure.h for it.
It works on raw record bytes, so whatever the contract says is ignored can hold garbage.  Fragment identity is ``graph_mirror.same_graph`` on
the mirror's own fragment records.

Also here: the hand-stated table of molecules with their cuts and labels (the pin: RDKit cannot run where the project runs) and the seeded
derived set that the CPU test checks for coverage and the GPU test compares on.
"""
from __future__ import annotations

import itertools
import math

import numpy as np

from tests import graph_mirror as GM, groups_mirror as G, structure_mirror as SM, substructure_mirror as Q, valence_mirror as VM

OK, UNUSABLE = 0, 3
W = SM.W
MAX_CUTS, ATTACH_TYPE, AROMATIC_ORDER = 28, 5, 4
H, C, N, O, F = range(5)
LABELS = (1, 3, 4, 5, 6, 7, 8, 9, 10, 13, 14, 15, 16)
# (x, y, bond order) in the header's order
RULES = [(1, 3, 1), (1, 5, 1), (1, 10, 1), (3, 4, 1), (3, 13, 1), (3, 14, 1), (3, 15, 1), (3, 16, 1), (4, 5, 1), (5, 14, 1), (5, 16, 1), (5, 13, 1),
         (5, 15, 1), (6, 13, 1), (6, 14, 1), (6, 15, 1), (6, 16, 1), (7, 7, 2), (8, 9, 1), (8, 10, 1), (8, 13, 1), (8, 14, 1), (8, 15, 1), (8, 16, 1),
         (9, 13, 1), (9, 14, 1), (9, 15, 1), (9, 16, 1), (10, 13, 1), (10, 14, 1), (10, 15, 1), (10, 16, 1), (13, 14, 1), (13, 15, 1), (13, 16, 1),
         (14, 14, 1), (14, 15, 1), (14, 16, 1), (15, 16, 1), (16, 16, 1)]
KEYS = ("env", "cuts", "fragment_of", "summary", "status")
SINGLE, DOUBLE, TRIPLE, AROMATIC = range(4)


class Analysis:
    """One record as the header sees it: ``env`` {atom: set of labels}, ``cuts`` [(a, b, label a, label b)], ``fragments`` [sorted atoms]."""

    def __init__(self, rec, n):
        g = Q.Graph(rec, n)
        self.usable = g.usable
        if not g.usable:
            return
        self.n, self.types, self.raw, self.orders, _, _ = VM.read(rec, n, VM.RECORD)
        t = self.types
        self.matchable, aromatic = list(g.matchable), set(g.aromatic)
        self.nbrs = {a: sorted(b for (x, b) in g.cls if x == a) for a in self.matchable}                # matchable neighbours
        self.kind = {ab: c % 4 for ab, c in g.cls.items()}
        self.ring = {ab: c >= 4 for ab, c in g.cls.items()}
        folded = [i for i in range(self.n) if i not in set(self.matchable)]
        atoms = [G.Atom(i, t, self.raw, self.orders) for i in range(self.n)]
        in_ring = {a: any(G.ring_bond(atoms, a, b) for b in atoms[a].nbrs) for a in self.matchable}    # on the graph of all atoms
        q = {a: atoms[a].q for a in self.matchable}

        def is_(a, elements, case):                                              # case: "upper" not aromatic, "lower" aromatic, "either"
            return t[a] in elements and (case == "either" or (a in aromatic) == (case == "lower"))

        def bonded(a, want):                                                     # the neighbours b of a with want(kind, ring bond, b)
            return [b for b in self.nbrs[a] if want(self.kind[a, b], self.ring[a, b], b)]

        def distinct(*lists):                                                    # one atom of every list, all different
            return any(len(set(pick)) == len(pick) for pick in itertools.product(*lists))

        def carbonyl(c):
            return is_(c, (C,), "upper") and any(self.kind[c, b] == DOUBLE and is_(b, (O,), "upper") for b in self.nbrs[c])

        def lactam(a):
            return is_(a, (N,), "upper") and in_ring[a] and bool(bonded(a, lambda k, r, b: r and carbonyl(b) and in_ring[b]))

        self.env = {}
        for a in self.matchable:
            D = len(self.nbrs[a])
            doubles = bonded(a, lambda k, r, b: k == DOUBLE)
            found = set()
            if is_(a, (C,), "upper"):
                to_O = bonded(a, lambda k, r, b: k == DOUBLE and is_(b, (O,), "upper"))
                if D == 3 and distinct(to_O, bonded(a, lambda k, r, b: is_(b, (C, N, O), "either"))):
                    found.add(1)
                if D != 1 and not doubles and bonded(a, lambda k, r, b: k == SINGLE and not r and is_(b, (C,), "either")):
                    found.add(4)
                if not in_ring[a] and D == 3 and distinct(to_O, bonded(a, lambda k, r, b: k == SINGLE and not r and is_(b, (C, N, O), "either"))):
                    found.add(6)
                if D in (2, 3) and bonded(a, lambda k, r, b: k == SINGLE and is_(b, (C,), "either")):
                    found.add(7)
                if not in_ring[a] and D != 1 and all(self.kind[a, b] == SINGLE for b in self.nbrs[a]):
                    found.add(8)
                if distinct(bonded(a, lambda k, r, b: k == SINGLE and r and is_(b, (C, N, O), "upper")),
                            bonded(a, lambda k, r, b: k == SINGLE and r and is_(b, (N, O), "upper"))):
                    found.add(13)
                ring_C = bonded(a, lambda k, r, b: k == SINGLE and r and is_(b, (C,), "upper"))
                if distinct(ring_C, ring_C):
                    found.add(15)
            if is_(a, (O,), "upper") and D == 2 and bonded(a, lambda k, r, b: k == SINGLE and not r and (is_(b, (C,), "either") or t[b] == H)):
                found.add(3)
            if is_(a, (N,), "upper"):
                if D != 1 and not doubles and not bonded(a, lambda k, r, b: k == SINGLE and is_(b, (N, O, F), "either")) and not lactam(a):
                    found.add(5)
                if in_ring[a] and distinct(bonded(a, lambda k, r, b: r and carbonyl(b)), bonded(a, lambda k, r, b: r and is_(b, (C, N, O), "upper"))):
                    found.add(10)
            if is_(a, (N,), "lower") and q[a] == 0:
                ring = bonded(a, lambda k, r, b: k == AROMATIC and is_(b, (C, N, O), "lower"))
                if distinct(ring, ring):
                    found.add(9)
            if is_(a, (C,), "lower"):
                if distinct(bonded(a, lambda k, r, b: k == AROMATIC and is_(b, (C, N, O), "lower")),
                            bonded(a, lambda k, r, b: k == AROMATIC and is_(b, (N, O), "lower"))):
                    found.add(14)
                ring_c = bonded(a, lambda k, r, b: k == AROMATIC and is_(b, (C,), "lower"))
                if distinct(ring_c, ring_c):
                    found.add(16)
            self.env[a] = found

        self.cuts = []
        for a in self.matchable:
            for b in self.nbrs[a]:
                if b < a or self.ring[a, b] or self.kind[a, b] not in (SINGLE, DOUBLE):
                    continue
                for x, y, order in RULES:
                    if order != self.kind[a, b] + 1:
                        continue
                    forward, reverse = x in self.env[a] and y in self.env[b], y in self.env[a] and x in self.env[b]
                    if forward or reverse:
                        self.cuts.append((a, b, x if forward else y, x if reverse else y))
                        break
        cut = {frozenset(c[:2]) for c in self.cuts}
        self.components = self._pieces(set())
        pieces = self._pieces(cut)
        owner = {a: k for k, piece in enumerate(pieces) for a in piece}
        for h in folded:                                                         # a folded hydrogen goes with its one neighbour
            pieces[owner[atoms[h].nbrs[0]]].append(h)
        self.fragments = [sorted(piece) for piece in pieces]
        self.aromatic_bond = {ab for ab, k in self.kind.items() if k == AROMATIC}

    def _pieces(self, without):
        """The components of the matchable graph without the bonds of ``without``, by ascending lowest atom."""
        seen, out = set(), []
        for s in self.matchable:
            if s in seen:
                continue
            seen.add(s)
            piece, stack = [], [s]
            while stack:
                u = stack.pop()
                piece.append(u)
                for v in self.nbrs[u]:
                    if v not in seen and frozenset((u, v)) not in without:
                        seen.add(v)
                        stack.append(v)
            out.append(piece)
        return out


def analyse(rec, n, found=None):
    """One row of ``dsb_brics_records``: dict(env [29], cuts [(a, b, la, lb)], fragment_of [29], summary (4), status)."""
    A = Analysis(rec, n) if found is None else found
    if not A.usable:
        return dict(env=[0] * W, cuts=[], fragment_of=[0xff] * W, summary=(0, 0, 0, 0), status=UNUSABLE)
    env = [sum(1 << e for e in A.env.get(i, ())) for i in range(W)]
    fragment_of = [0xff] * W
    for f, atoms in enumerate(A.fragments):
        for i in atoms:
            fragment_of[i] = f
    return dict(env=env, cuts=sorted(A.cuts), fragment_of=fragment_of,
                summary=(len(A.matchable), len(A.cuts), len(A.fragments), max(len(f) for f in A.fragments)), status=OK)


def analyse_table(rec, n):
    return [analyse(r, k) for r, k in zip(np.asarray(rec), np.asarray(n))]


def as_arrays(rows):
    """The rows of ``analyse_table`` as the five arrays of the kernel."""
    P = len(rows)
    cuts = np.full((P, MAX_CUTS, 4), 0xff, np.uint8)
    for p, r in enumerate(rows):
        for k, c in enumerate(r["cuts"]):
            cuts[p, k] = c
    return (np.array([r["env"] for r in rows], np.int32).reshape(P, W), cuts, np.array([r["fragment_of"] for r in rows], np.uint8).reshape(P, W),
            np.array([r["summary"] for r in rows], np.int32).reshape(P, 4), np.array([r["status"] for r in rows], np.uint8))


def fragment_rows(rec, n, aromatic=True, found=None):
    """The rows of ``dsb_brics_fragment_records`` of one record: [(record bytes uint8 [1248], out_n, source [29])], none for an unusable one."""
    A = Analysis(rec, n) if found is None else found
    if not A.usable:
        return []
    rec = np.ascontiguousarray(np.asarray(rec, np.uint8))
    pos_in = rec[SM.POS:SM.TYPE].reshape(W, 12)
    rows = []
    for atoms in A.fragments:
        inside = set(atoms)
        ends = sorted([(b, a, la) for a, b, la, lb in A.cuts if a in inside] + [(a, b, lb) for a, b, la, lb in A.cuts if b in inside])      # (outside, inside, label)
        out, source = np.zeros(SM.RECORD_BYTES, np.uint8), [0xff] * W
        pos, bond = out[SM.POS:SM.TYPE].reshape(W, 12), out[SM.BOND:SM.BOND_END].reshape(W, W)
        slot = {a: r for r, a in enumerate(atoms)}
        for a, r in slot.items():
            pos[r] = pos_in[a]
            out[SM.TYPE + r] = A.types[a]
            out[SM.FC + r] = np.array(VM.applied_charge(A.types[a], A.raw[a]), np.int8).view(np.uint8)
            source[r] = a
            for b, s in slot.items():
                if A.orders[a][b]:
                    bond[r, s] = AROMATIC_ORDER if aromatic and (a, b) in A.aromatic_bond else A.orders[a][b]
        for k, (outside, a, label) in enumerate(ends):
            r = len(atoms) + k
            pos[r] = pos_in[outside]
            out[SM.TYPE + r], out[SM.FC + r], source[r] = ATTACH_TYPE, label, outside
            bond[r, slot[a]] = bond[slot[a], r] = A.orders[a][outside]
        rows.append((out, len(atoms) + len(ends), source))
    return rows


def fragment_table(rec, n, aromatic=True):
    """(out_rec [F, 1248], out_n [F], out_owner [F], out_source [F, 29]) of a record table, as the kernel writes them with the caller's prefix sum."""
    recs, counts, owner, source = [], [], [], []
    for p, (r, k) in enumerate(zip(np.asarray(rec), np.asarray(n))):
        for out, m, src in fragment_rows(r, k, aromatic):
            recs.append(out)
            counts.append(m)
            owner.append(p)
            source.append(src)
    F = len(recs)
    return (np.stack(recs) if F else np.zeros((0, SM.RECORD_BYTES), np.uint8), np.array(counts, np.int32), np.array(owner, np.int64),
            np.array(source, np.uint8).reshape(F, W))


def fragment_mols(rec, n, aromatic=True):
    """The fragments of one record as molecule dicts (attachment points included)."""
    return [SM.mol_from_record(out, m) for out, m, _ in fragment_rows(rec, n, aromatic)]


class Classes:
    """Molecules up to ``graph_mirror.same_graph``, numbered in the order they are first seen; a cheap invariant (atom count, the multiset of
    (type, charge), the multiset of bond bytes) keeps the searches short."""

    def __init__(self):
        self.mols, self.buckets = [], {}

    def find(self, mol):
        """The number of ``mol``'s class; a molecule not seen before opens one."""
        upper = np.triu(np.asarray(mol["bond"]), 1).ravel()
        key = (len(mol["type"]), tuple(sorted(zip(mol["type"].tolist(), (mol["fc"] & 255).tolist()))), tuple(sorted(upper[upper > 0].tolist())))
        bucket = self.buckets.setdefault(key, [])
        for c in bucket:
            if GM.same_graph(mol, self.mols[c]):
                return c
        self.mols.append(mol)
        bucket.append(len(self.mols) - 1)
        return bucket[-1]


def fragment_counts(rec, n, aromatic=True, classes=None):
    """(classes, counts {class: fragments}, [(owner, class)] of every fragment, cuts of every usable record); ``classes`` is extended in
    place, so that two sides counted one after the other share their class numbers."""
    classes = Classes() if classes is None else classes
    counts, of_fragment, cuts = {}, [], []
    for p, (r, k) in enumerate(zip(np.asarray(rec), np.asarray(n))):
        A = Analysis(r, k)
        if not A.usable:
            continue
        cuts.append(len(A.cuts))
        for out, m, _ in fragment_rows(r, k, aromatic, A):
            c = classes.find(SM.mol_from_record(out, m))
            counts[c] = counts.get(c, 0) + 1
            of_fragment.append((p, c))
    return classes, counts, of_fragment, cuts


def cosine(g, t):
    """Frag of two count tables {fragment: count}: exact integer sums, one division and one square root."""
    dot, gg, tt = sum(c * t[k] for k, c in g.items() if k in t), sum(c * c for c in g.values()), sum(c * c for c in t.values())
    return dot / math.sqrt(gg * tt) if gg and tt else float("nan")


def fragment_metric(gen, test, aromatic=True):
    """What ``get_fragment_metric(test, unique=False, aromatic)(gen)`` gives, the class ids as this mirror numbers them."""
    classes, t, _, _ = fragment_counts(*test, aromatic)
    _, g, of_fragment, cuts = fragment_counts(*gen, aromatic, classes)
    return dict(frag=cosine(g, t), n_generated=len(gen[1]), n_test=len(test[1]), fragments_generated=sum(g.values()), fragments_test=sum(t.values()),
                distinct_generated=len(g), distinct_test=len(t), shared=len(set(g) & set(t)), mean_cuts=sum(cuts) / len(cuts) if cuts else float("nan"),
                fragment_class=[c for _, c in of_fragment], owner=[p for p, _ in of_fragment])


# ------------------------------------------------------------------------------------------------------------------ molecules

def _chain(k, start=0):
    return [(start + i, start + i + 1, 1) for i in range(k - 1)]


def _cycle(*atoms, order=1):
    return [(a, b, order) for a, b in zip(atoms, atoms[1:] + atoms[:1])]


_PYRROLE = [(0, 1, 1), (1, 2, 2), (2, 3, 1), (3, 4, 2), (4, 0, 1)]


def hand_table():
    """[(name, molecule, cuts)] with cuts = [(a, b, label of a, label of b)], a < b: stated by hand from the header's environments and rule
    order, not computed.  The heavy atoms come first in every molecule (G.molecule appends the hydrogens)."""
    mol, benz = G.molecule, G._ring(True)
    return [
        ("propyl ethyl ether", mol("CCCOCC", _chain(6), [3, 2, 2, 0, 2, 3]), [(2, 3, 4, 3), (3, 4, 3, 4)]),
        ("dimethyl ether", mol("COC", _chain(3), [3, 0, 3]), []),
        ("ethanol", mol("CCO", _chain(3), [3, 2, 1]), []),
        ("toluene", mol("CCCCCCC", benz + [(0, 6, 1)], [0, 1, 1, 1, 1, 1, 3]), []),
        ("pentan-3-one", mol("CCCCCO", _chain(5) + [(2, 5, 2)], [3, 2, 0, 2, 3, 0]), []),
        ("ethene", mol("CC", [(0, 1, 2)], [2, 2]), []),
        ("cyclohexene", mol("CCCCCC", [(0, 1, 2)] + _chain(6)[1:] + [(5, 0, 1)], [1, 1, 2, 2, 2, 2]), []),
        ("CCNOC", mol("CCNOC", _chain(5), [3, 2, 1, 0, 3]), []),
        ("CC=NCC", mol("CCNCC", [(0, 1, 1), (1, 2, 2), (2, 3, 1), (3, 4, 1)], [3, 1, 0, 2, 3]), []),
        ("N-methylacetamide", mol("CCONC", [(0, 1, 1), (1, 2, 2), (1, 3, 1), (3, 4, 1)], [3, 0, 0, 1, 3]), [(1, 3, 1, 5)]),
        ("methyl acetate", mol("CCOOC", [(0, 1, 1), (1, 2, 2), (1, 3, 1), (3, 4, 1)], [3, 0, 0, 0, 3]), [(1, 3, 1, 3)]),
        ("ethyl acetate", mol("CCOOCC", [(0, 1, 1), (1, 2, 2), (1, 3, 1), (3, 4, 1), (4, 5, 1)], [3, 0, 0, 0, 2, 3]), [(1, 3, 1, 3), (3, 4, 3, 4)]),
        ("N-ethylacetamide", mol("CCONCC", [(0, 1, 1), (1, 2, 2), (1, 3, 1), (3, 4, 1), (4, 5, 1)], [3, 0, 0, 1, 2, 3]), [(1, 3, 1, 5), (3, 4, 5, 4)]),
        ("diethylamine", mol("CCNCC", _chain(5), [3, 2, 1, 2, 3]), [(1, 2, 4, 5), (2, 3, 5, 4)]),
        ("ethylbenzene", mol("CCCCCCCC", benz + [(0, 6, 1), (6, 7, 1)], [0, 1, 1, 1, 1, 1, 2, 3]), [(0, 6, 16, 8)]),
        ("anisole", mol("CCCCCCOC", benz + [(0, 6, 1), (6, 7, 1)], [0, 1, 1, 1, 1, 1, 0, 3]), [(0, 6, 16, 3)]),
        ("biphenyl", Q._biphenyl(), [(0, 6, 16, 16)]),
        ("2-ethylpyridine", mol("NCCCCCCC", benz + [(1, 6, 1), (6, 7, 1)], [0, 0, 1, 1, 1, 1, 2, 3]), [(1, 6, 14, 8)]),
        ("1-ethylpyrrole", mol("NCCCCCC", _PYRROLE + [(0, 5, 1), (5, 6, 1)], [0, 1, 1, 1, 1, 2, 3]), [(0, 5, 9, 8)]),
        ("but-2-ene", mol("CCCC", [(0, 1, 1), (1, 2, 2), (2, 3, 1)], [3, 1, 1, 3]), [(1, 2, 7, 7)]),
        ("ethylcyclopropane", mol("CCCCC", _cycle(0, 1, 2) + [(0, 3, 1), (3, 4, 1)], [1, 2, 2, 2, 3]), [(0, 3, 15, 8)]),
        ("ethoxycyclopropane", mol("CCCOCC", _cycle(0, 1, 2) + [(0, 3, 1), (3, 4, 1), (4, 5, 1)], [1, 2, 2, 0, 2, 3]), [(0, 3, 15, 3), (3, 4, 3, 4)]),
        # the ring amide bond 0-1 is a ring bond and is not cut; the lactam N is L10 and not L5
        ("1-ethylpyrrolidin-2-one", mol("NCCCCOCC", _cycle(0, 1, 2, 3, 4) + [(1, 5, 2), (0, 6, 1), (6, 7, 1)], [0, 0, 2, 2, 2, 0, 2, 3]), [(0, 6, 10, 8)]),
        ("2-ethyloxolane", mol("OCCCCCC", _cycle(0, 1, 2, 3, 4) + [(1, 5, 1), (5, 6, 1)], [0, 1, 2, 2, 2, 2, 3]), [(1, 5, 13, 8)]),
        ("acetophenone", mol("CCCCCCCOC", benz + [(0, 6, 1), (6, 7, 2), (6, 8, 1)], [0, 1, 1, 1, 1, 1, 0, 0, 3]), [(0, 6, 16, 6)]),
        # carbon 0 is in L13 and in L15; rule 3-13 precedes 3-15
        ("1-methoxy-7-oxabicyclo[2.2.1]heptane", mol("CCCCCCOOC", _cycle(0, 1, 2, 3, 4, 5) + [(0, 6, 1), (3, 6, 1), (0, 7, 1), (7, 8, 1)],
                                                     [0, 2, 2, 1, 2, 2, 0, 0, 3]), [(0, 7, 13, 3)]),
        # both orientations of 13-15: carbons 0 and 4 are each in L13 (ring O, ring C) and in L15 (two ring C), so both ends get 13
        ("1,1'-bi(2-oxabicyclo[1.1.0]butyl)", mol("COCCCOCC", [(0, 1, 1), (1, 2, 1), (0, 2, 1), (0, 3, 1), (2, 3, 1), (4, 5, 1), (5, 6, 1), (4, 6, 1), (4, 7, 1),
                                                               (6, 7, 1), (0, 4, 1)], [0, 0, 1, 2, 0, 0, 1, 2]), [(0, 4, 13, 13)]),
        ("N-methylacetamide and but-2-ene", mol("CCONCCCCC", [(0, 1, 1), (1, 2, 2), (1, 3, 1), (3, 4, 1), (5, 6, 1), (6, 7, 2), (7, 8, 1)],
                                                [3, 0, 0, 1, 3, 3, 1, 1, 3]), [(1, 3, 1, 5), (6, 7, 7, 7)]),
        # atom 3 is a hydrogen with two bonds: matchable, in no environment; the oxygen is L3 with D = 2
        ("ethanol whose hydroxyl hydrogen bridges to ethyl", mol("CCOHCC", _chain(6), [3, 2, 0, 0, 2, 3]), [(1, 2, 4, 3)]),
    ]


def named(name):
    return [mol for nm, mol, _ in hand_table() if nm == name][0]


def renumbered(mol, perm):
    """New atom i is old atom perm[i]."""
    return dict(pos=mol["pos"][perm], type=mol["type"][perm].copy(), fc=mol["fc"][perm].copy(), bond=mol["bond"][np.ix_(perm, perm)].copy())


def moved_cuts(cuts, perm):
    """The stated cuts of a molecule after ``renumbered(mol, perm)``."""
    new = {int(old): i for i, old in enumerate(perm)}
    return sorted((new[a], new[b], la, lb) if new[a] < new[b] else (new[b], new[a], lb, la) for a, b, la, lb in cuts)


def kekule_pairs():
    """[(name, drawing, other drawing)]: the two Kekule drawings of aromatic molecules whose ring fragment no symmetry maps onto itself with
    the orders exchanged, atoms numbered alike: the ring fragments differ with Kekule orders and are one with the aromatic byte."""
    mol, a, b = G.molecule, G._ring(True), G._ring(False)
    out = []
    for name, elements, tail, hydrogens in (
            ("2-ethylpyridine", "NCCCCCCC", [(1, 6, 1), (6, 7, 1)], [0, 0, 1, 1, 1, 1, 2, 3]),
            ("3-ethylpyridine", "NCCCCCCC", [(2, 6, 1), (6, 7, 1)], [0, 1, 0, 1, 1, 1, 2, 3]),
            ("2-methoxypyridine", "NCCCCCOC", [(1, 6, 1), (6, 7, 1)], [0, 0, 1, 1, 1, 1, 0, 3]),
            ("2-ethyl-1-fluorobenzene", "CCCCCCCCF", [(0, 6, 1), (6, 7, 1), (1, 8, 1)], [0, 0, 1, 1, 1, 1, 2, 3, 0]),
            ("2-ethylphenol", "CCCCCCCCO", [(0, 6, 1), (6, 7, 1), (1, 8, 1)], [0, 0, 1, 1, 1, 1, 2, 3, 1]),
            ("3-ethylaniline", "CCCCCCCCN", [(0, 6, 1), (6, 7, 1), (2, 8, 1)], [0, 1, 0, 1, 1, 1, 2, 3, 2]),
            ("2-acetylpyridine", "NCCCCCCOC", [(1, 6, 1), (6, 7, 2), (6, 8, 1)], [0, 0, 1, 1, 1, 1, 0, 0, 3]),
            ("2-phenylpyridine", "NCCCCC" + "C" * 6, [(6 + i, 6 + j, o) for i, j, o in a] + [(1, 6, 1)], [0, 0, 1, 1, 1, 1] + [0, 1, 1, 1, 1, 1])):
        out.append((name, mol(elements, a + tail, hydrogens), mol(elements, b + tail, hydrogens)))
    return out


# first atom replaces the hydrogen; (type, parent inside the group or -1 for the atom the hydrogen was on, order)
_GROUPS = {
    "F": [(F, -1, 1)],
    "OH": [(O, -1, 1), (H, 0, 1)],
    "NH2": [(N, -1, 1), (H, 0, 1), (H, 0, 1)],
    "CH3": [(C, -1, 1), (H, 0, 1), (H, 0, 1), (H, 0, 1)],
    "CHO": [(C, -1, 1), (O, 0, 2), (H, 0, 1)],
    "C2H5": [(C, -1, 1), (H, 0, 1), (H, 0, 1), (C, 0, 1), (H, 3, 1), (H, 3, 1), (H, 3, 1)],
    "OCH3": [(O, -1, 1), (C, 0, 1), (H, 1, 1), (H, 1, 1), (H, 1, 1)],
    "NHCH3": [(N, -1, 1), (H, 0, 1), (C, 0, 1), (H, 2, 1), (H, 2, 1), (H, 2, 1)],
    "COCH3": [(C, -1, 1), (O, 0, 2), (C, 0, 1), (H, 2, 1), (H, 2, 1), (H, 2, 1)],
}
SUBSTITUENTS = tuple(_GROUPS)


def substituted(mol, h, group):
    """``mol`` with its hydrogen atom ``h`` replaced by ``group``; the further atoms of the group are appended."""
    types, fc = [int(t) for t in mol["type"]], [int(c) for c in mol["fc"]]
    n = len(types)
    assert types[h] == H
    bonds = [(i, j, int(mol["bond"][i, j])) for i in range(n) for j in range(i + 1, n) if mol["bond"][i, j]]
    spec = _GROUPS[group]
    index = [h] + list(range(n, n + len(spec) - 1))
    types[h] = spec[0][0]
    for k, (t, parent, order) in enumerate(spec[1:], start=1):
        types.append(t)
        fc.append(0)
        bonds.append((index[parent], index[k], order))
    return VM.molecule(types, bonds, fc=fc)


def _grown(mol, rng, twins=()):
    """``mol`` (and its ``twins``, numbered alike) with one hydrogen, half of the time a second one, replaced by a substituent while the
    molecule still fits a record."""
    out = [mol, *twins]
    for _ in range(1 + int(rng.integers(2))):
        hs = np.nonzero((np.asarray(out[0]["type"]) == H) & ((np.asarray(out[0]["bond"]) > 0).sum(1) == 1))[0]      # not a bridging hydrogen
        group = SUBSTITUENTS[int(rng.integers(len(SUBSTITUENTS)))]
        if hs.size == 0:
            break
        h = int(rng.choice(hs))
        if len(out[0]["type"]) + len(_GROUPS[group]) - 1 <= W:
            out = [substituted(m, h, group) for m in out]
    return out


def derived_set(seed=20261020, grown=6, pairs=2, closed=70):
    """About 300 molecules, fixed by the seed: every molecule of the table with substituents grown on, ``grown`` times each; both Kekule
    drawings of every molecule of ``kekule_pairs`` as they are and grown alike ``pairs`` times (the two drawings are neighbours in the list);
    ``closed`` molecules of ``graph_mirror.random_molecule`` (0-3 ring closures, random charges), every other one with its hydrogens turned into
    carbons."""
    rng = np.random.default_rng(seed)
    out = []
    for name, mol, _ in hand_table():
        for _ in range(grown):
            out += _grown(mol, rng)
    for name, a, b in kekule_pairs():
        out += [a, b]
        for _ in range(pairs):
            out += _grown(a, rng, (b,))
    for k in range(closed):
        mol = GM.random_molecule(rng, int(rng.integers(6, 24)))
        if k % 2:
            mol["type"] = np.where(mol["type"] == H, C, mol["type"])
        out.append(mol)
    return out
