"""CPU yardstick of ``dsg_group_records`` and ``dsg_group_similarity_records`` in plain Python, written from the text of
include/diffspectra_groups.h and not from the kernel: per-atom quantities (applied charge, implicit hydrogens, X, Ht), ring bonds by a
breadth-first search without the bond, aromatic cycles by a depth-first enumeration of the simple cycles of 5 and 6 atoms with the electron
rule applied to each, and the 17 predicates as nested searches over atoms.  It works on raw record bytes, so whatever the contract says is
ignored can hold garbage.

Also here: the hand-stated table of molecules (the pin: RDKit cannot run where the project runs), their second Kekule drawings, and the seeded
generator of substituted molecules that the CPU test checks for coverage and the GPU test compares on.
"""
from __future__ import annotations

import numpy as np
import torch

from tests import valence_mirror as VM

OK, UNUSABLE, INVALID = 0, 2, 3
NAMES = ("alkane", "alkene", "alkyne", "arene", "alcohol", "ether", "aldehyde", "ketone", "carboxylic acid", "ester", "haloalkane", "acyl halide",
         "amine", "amide", "nitrile", "sulfide", "thiol")
H, C, N, O, F = range(5)


class Atom:
    """The header's per-atom quantities."""

    def __init__(self, i, types, raw, orders):
        row = orders[i]
        self.i, self.t = i, types[i]
        self.q = VM.applied_charge(self.t, raw[i])
        self.nbrs = [j for j, b in enumerate(row) if b > 0]
        self.valence = sum(row)
        self.D = len(self.nbrs)
        self.hi = max(0, VM.VMAX[self.t, self.q] - self.valence)
        self.X = self.D + self.hi
        self.Ht = sum(1 for j in self.nbrs if types[j] == H) + self.hi
        self.by_order = {o: [j for j, b in enumerate(row) if b == o] for o in (1, 2, 3)}
        self.dbl, self.trp = len(self.by_order[2]), len(self.by_order[3])


def ring_bond(atoms, a, b):
    """b reached from a over bonds of order > 0 without the bond a-b."""
    seen, queue = {a}, [a]
    while queue:
        u = queue.pop(0)
        for v in atoms[u].nbrs:
            if {u, v} == {a, b} or v in seen:
                continue
            if v == b:
                return True
            seen.add(v)
            queue.append(v)
    return False


def never_candidate(A):
    return A.t in (H, F) or A.trp > 0 or A.dbl >= 2 or A.X > 3


def electrons(atoms, A, cycle):
    """The electron count of atom A as a candidate of ``cycle`` (a set of atoms), None when it is none."""
    if never_candidate(A):
        return None
    if A.t in (C, N) and A.dbl == 1:
        fits = (A.X == 3 and A.q == 0) if A.t == C else ((A.X == 2 and A.q == 0) or (A.X == 3 and A.q == 1))
        if not fits:
            return None
        p = A.by_order[2][0]
        if p in cycle or ring_bond(atoms, A.i, p):
            return 1
        return 0 if atoms[p].t in (N, O) else None
    if A.dbl != 0:
        return None
    if A.t == C:
        return {-1: 2, 1: 0}.get(A.q) if A.X == 3 else None
    if A.t == N:
        return 2 if (A.X == 3 and A.q == 0) or (A.X == 2 and A.q == -1) else None
    return 2 if A.X == 2 and A.q == 0 else None                                # O


def aromatic_atoms(atoms):
    """The atoms that lie on an aromatic simple cycle of 5 or 6 atoms.  Every cycle is listed from its lowest atom; atoms that are never
    candidates are not walked (a cycle through one is not aromatic whatever the rest), which also bounds the search: the others have X <= 3."""
    walk = [not never_candidate(A) for A in atoms]
    found = set()

    def extend(path):
        last = atoms[path[-1]]
        if len(path) in (5, 6) and path[0] in last.nbrs:
            cycle = set(path)
            counts = [electrons(atoms, atoms[i], cycle) for i in path]
            if None not in counts and sum(counts) == 6:
                found.update(cycle)
        if len(path) < 6:
            for v in last.nbrs:
                if v > path[0] and walk[v] and v not in path:
                    extend(path + [v])
    for s in range(len(atoms)):
        if walk[s]:
            extend([s])
    return found


def group_bits(atoms, aromatic):
    """The predicates of the header, one search each."""
    al = lambda i: i not in aromatic
    is_c = lambda i: atoms[i].t == C
    al_c = lambda i: is_c(i) and al(i)
    al_o = lambda i: atoms[i].t == O and al(i)
    carbonyl = lambda A, x1=False: any(al_o(o) and (not x1 or atoms[o].X == 1) for o in A.by_order[2])
    single_c = lambda A: [j for j in A.by_order[1] if is_c(j)]
    has = set()
    for A in atoms:
        i, t = A.i, A.t
        if t == C and al(i):
            if A.X == 4:
                has.add("alkane")
            if A.X == 3 and any(al_c(j) and atoms[j].X == 3 for j in A.by_order[2]):
                has.add("alkene")
            if A.X == 2 and any(al_c(j) for j in A.by_order[3]):
                has.add("alkyne")
            if A.X == 3 and carbonyl(A):
                if A.Ht == 1 and single_c(A):
                    has.add("aldehyde")
                if len(single_c(A)) >= 2:
                    has.add("ketone")
                if any(al_o(o) and atoms[o].X == 2 and atoms[o].Ht == 1 for o in A.by_order[1]):
                    has.add("carboxylic acid")
                for o in A.by_order[1]:
                    if al_o(o) and atoms[o].X == 2 and atoms[o].Ht == 0:
                        if any(r != r2 for r in single_c(A) for r2 in single_c(atoms[o]) if r2 != i):
                            has.add("ester")
            if A.X == 3 and carbonyl(A, x1=True) and any(atoms[j].t == F for j in A.by_order[1]):
                has.add("acyl halide")
        if t == C and not al(i):
            has.add("arene")
        if t == O and al(i):
            if A.X == 2 and A.Ht == 1 and single_c(A):
                has.add("alcohol")
            if A.D == 2 and len(single_c(A)) == 2:
                has.add("ether")
        if t == F and single_c(A):
            has.add("haloalkane")
        if t == N and al(i):
            if A.X == 3 and not any(al_c(j) and carbonyl(atoms[j]) for j in A.by_order[1]):
                has.add("amine")
            if A.X == 3 and any(al_c(j) and atoms[j].X == 3 and carbonyl(atoms[j], x1=True) and single_c(atoms[j]) for j in A.by_order[1]):
                has.add("amide")
            if A.X == 1 and any(al_c(j) and atoms[j].X == 2 for j in A.by_order[3]):
                has.add("nitrile")
    return sum(1 << NAMES.index(name) for name in has)


def analyse(rec, n):
    """One row of ``dsg_group_records``: dict(groups, aromatic_mask, status)."""
    n, types, raw, orders, usable, _ = VM.read(rec, n, VM.RECORD)
    if not usable:
        return dict(groups=0, aromatic_mask=0, status=UNUSABLE)
    atoms = [Atom(i, types, raw, orders) for i in range(n)]
    aromatic = aromatic_atoms(atoms)
    return dict(groups=group_bits(atoms, aromatic), aromatic_mask=VM.bits(aromatic), status=OK)


def analyse_table(rec, n):
    return [analyse(r, k) for r, k in zip(np.asarray(rec), np.asarray(n))]


def has_plain_ring(rec, n):
    """A ring bond with an end that is not aromatic (the coverage condition's "non-aromatic ring")."""
    k, types, raw, orders, usable, _ = VM.read(rec, n, VM.RECORD)
    if not usable:
        return False
    atoms = [Atom(i, types, raw, orders) for i in range(k)]
    aromatic = aromatic_atoms(atoms)
    return any(ring_bond(atoms, a, b) for a in range(k) for b in atoms[a].nbrs if a < b and not (a in aromatic and b in aromatic))


def similarity_pair(prb, ref):
    """One row of ``dsg_group_similarity_records`` from two analysed rows: dict(common, either, groups (2), status)."""
    if prb["status"] != OK or ref["status"] != OK:
        return dict(common=-1, either=-1, groups=(0, 0), status=UNUSABLE)
    gp, gr = prb["groups"], ref["groups"]
    return dict(common=bin(gp & gr).count("1"), either=bin(gp | gr).count("1"), groups=(gp, gr), status=OK)


def similarity_table(prb_rec, prb_n, ref_rec, ref_n, ref_index=None):
    rows = []
    for p in range(len(prb_n)):
        r = p if ref_index is None else int(ref_index[p])
        if not 0 <= r < len(ref_n):
            rows.append(dict(common=-1, either=-1, groups=(0, 0), status=INVALID))
        else:
            rows.append(similarity_pair(analyse(prb_rec[p], prb_n[p]), analyse(ref_rec[r], ref_n[r])))
    return rows


def jaccard(row):
    return 1.0 if row["either"] == 0 else row["common"] / row["either"]


def names_of(word):
    return {name for g, name in enumerate(NAMES) if (word >> g) & 1}


# ------------------------------------------------------------------------------------------------------------------ molecules

def molecule(elements, bonds, hydrogens, fc=None):
    """Molecule dict from the heavy atoms (a string such as 'CCO'), their bonds ``[(i, j, order)]`` and the EXPLICIT hydrogens of every heavy
    atom, which are appended after the heavy atoms in their order."""
    types, all_bonds = ["HCNOF".index(e) for e in elements], list(bonds)
    charges = list(fc) if fc is not None else [0] * len(types)
    for i, count in enumerate(hydrogens):
        for _ in range(count):
            all_bonds.append((i, len(types), 1))
            types.append(H)
            charges.append(0)
    return VM.molecule(types, all_bonds, fc=charges)


def _ring(first_double, size=6):
    """Bonds of a ring 0..size-1 with alternating orders; ``first_double`` says whether the bond 0-1 is the double one."""
    return [(i, (i + 1) % size, 2 if (i % 2 == 0) == first_double else 1) for i in range(size)]


_NAPHTHALENE = ([(0, 1, 2), (1, 2, 1), (2, 3, 2), (3, 8, 1), (8, 9, 2), (9, 0, 1), (3, 4, 1), (4, 5, 2), (5, 6, 1), (6, 7, 2), (7, 8, 1)],
                [(0, 1, 1), (1, 2, 2), (2, 3, 1), (3, 8, 2), (8, 9, 1), (9, 0, 2), (3, 4, 1), (4, 5, 2), (5, 6, 1), (6, 7, 2), (7, 8, 1)])
_NAPHTHALENE_H = [1, 1, 1, 0, 1, 1, 1, 1, 0, 1]


def hand_table():
    """[(name, molecule, groups expected, aromatic heavy atoms expected)]: stated by hand from the header's definitions and ordinary
    chemistry, not computed."""
    benz = _ring(True)
    six = set(range(6))
    rows = [
        ("methane", molecule("C", [], [4]), {"alkane"}, set()),
        ("ethanol", molecule("CCO", [(0, 1, 1), (1, 2, 1)], [3, 2, 1]), {"alkane", "alcohol"}, set()),
        ("dimethyl ether", molecule("COC", [(0, 1, 1), (1, 2, 1)], [3, 0, 3]), {"alkane", "ether"}, set()),
        ("acetaldehyde", molecule("CCO", [(0, 1, 1), (1, 2, 2)], [3, 1, 0]), {"alkane", "aldehyde"}, set()),
        ("acetone", molecule("CCCO", [(0, 1, 1), (1, 2, 1), (1, 3, 2)], [3, 0, 3, 0]), {"alkane", "ketone"}, set()),
        ("acetic acid", molecule("CCOO", [(0, 1, 1), (1, 2, 2), (1, 3, 1)], [3, 0, 0, 1]), {"alkane", "alcohol", "carboxylic acid"}, set()),
        ("methyl acetate", molecule("CCOOC", [(0, 1, 1), (1, 2, 2), (1, 3, 1), (3, 4, 1)], [3, 0, 0, 0, 3]), {"alkane", "ether", "ester"}, set()),
        ("methyl formate", molecule("COOC", [(0, 1, 2), (0, 2, 1), (2, 3, 1)], [1, 0, 0, 3]), {"alkane", "ether"}, set()),
        ("fluoromethane", molecule("CF", [(0, 1, 1)], [3, 0]), {"alkane", "haloalkane"}, set()),
        ("acetyl fluoride", molecule("CCOF", [(0, 1, 1), (1, 2, 2), (1, 3, 1)], [3, 0, 0, 0]), {"alkane", "haloalkane", "acyl halide"}, set()),
        ("methylamine", molecule("CN", [(0, 1, 1)], [3, 2]), {"alkane", "amine"}, set()),
        ("acetamide", molecule("CCON", [(0, 1, 1), (1, 2, 2), (1, 3, 1)], [3, 0, 0, 2]), {"alkane", "amide"}, set()),
        ("nitromethane (N+, O-)", molecule("CNOO", [(0, 1, 1), (1, 2, 2), (1, 3, 1)], [3, 0, 0, 0], fc=[0, 1, 0, -1]), {"alkane", "amine"}, set()),
        ("acetonitrile", molecule("CCN", [(0, 1, 1), (1, 2, 3)], [3, 0, 0]), {"alkane", "nitrile"}, set()),
        ("HCN", molecule("CN", [(0, 1, 3)], [1, 0]), {"nitrile"}, set()),
        ("propyne", molecule("CCC", [(0, 1, 1), (1, 2, 3)], [3, 0, 1]), {"alkane", "alkyne"}, set()),
        ("ethyne", molecule("CC", [(0, 1, 3)], [1, 1]), {"alkyne"}, set()),
        ("ethene", molecule("CC", [(0, 1, 2)], [2, 2]), {"alkene"}, set()),
        ("fluoroethene", molecule("CCF", [(0, 1, 2), (1, 2, 1)], [2, 1, 0]), {"alkene", "haloalkane"}, set()),
        ("benzene", molecule("CCCCCC", benz, [1] * 6), {"arene"}, six),
        ("pyridine", molecule("NCCCCC", benz, [0, 1, 1, 1, 1, 1]), {"arene"}, six),
        ("pyrrole", molecule("NCCCC", [(0, 1, 1), (1, 2, 2), (2, 3, 1), (3, 4, 2), (4, 0, 1)], [1] * 5), {"arene"}, set(range(5))),
        ("furan", molecule("OCCCC", [(0, 1, 1), (1, 2, 2), (2, 3, 1), (3, 4, 2), (4, 0, 1)], [0, 1, 1, 1, 1]), {"arene"}, set(range(5))),
        ("imidazole", molecule("NCNCC", [(0, 1, 1), (1, 2, 2), (2, 3, 1), (3, 4, 2), (4, 0, 1)], [1, 1, 0, 1, 1]), {"arene"}, set(range(5))),
        ("2-pyridone", molecule("NCCCCCO", [(0, 1, 1), (1, 6, 2), (1, 2, 1), (2, 3, 2), (3, 4, 1), (4, 5, 2), (5, 0, 1)], [1, 0, 1, 1, 1, 1, 0]), {"arene"}, six),
        ("indole", molecule("NCCCCCCCC", [(0, 1, 1), (1, 2, 2), (2, 3, 1), (3, 8, 2), (8, 0, 1), (3, 4, 1), (4, 5, 2), (5, 6, 1), (6, 7, 2), (7, 8, 1)],
                            [1, 1, 1, 0, 1, 1, 1, 1, 0]), {"arene"}, set(range(9))),
        ("naphthalene", molecule("C" * 10, _NAPHTHALENE[0], _NAPHTHALENE_H), {"arene"}, set(range(10))),
        ("toluene", molecule("CCCCCCC", benz + [(0, 6, 1)], [0, 1, 1, 1, 1, 1, 3]), {"alkane", "arene"}, six),
        ("phenol", molecule("CCCCCCO", benz + [(0, 6, 1)], [0, 1, 1, 1, 1, 1, 1]), {"arene", "alcohol"}, six),
        ("anisole", molecule("CCCCCCOC", benz + [(0, 6, 1), (6, 7, 1)], [0, 1, 1, 1, 1, 1, 0, 3]), {"alkane", "arene", "ether"}, six),
        ("aniline", molecule("CCCCCCN", benz + [(0, 6, 1)], [0, 1, 1, 1, 1, 1, 2]), {"arene", "amine"}, six),
        ("fluorobenzene", molecule("CCCCCCF", benz + [(0, 6, 1)], [0, 1, 1, 1, 1, 1, 0]), {"arene", "haloalkane"}, six),
        ("cyclopentadiene", molecule("CCCCC", [(0, 1, 1), (1, 2, 2), (2, 3, 1), (3, 4, 2), (4, 0, 1)], [2, 1, 1, 1, 1]), {"alkane", "alkene"}, set()),
        ("4H-pyran", molecule("OCCCCC", [(0, 1, 1), (1, 2, 2), (2, 3, 1), (3, 4, 1), (4, 5, 2), (5, 0, 1)], [0, 1, 1, 2, 1, 1]),
         {"alkane", "alkene", "ether"}, set()),
        ("p-benzoquinone", molecule("CCCCCCOO", [(0, 1, 1), (1, 2, 2), (2, 3, 1), (3, 4, 1), (4, 5, 2), (5, 0, 1), (0, 6, 2), (3, 7, 2)],
                                    [0, 1, 1, 0, 1, 1, 0, 0]), {"alkene", "ketone"}, set()),
        ("fulvene", molecule("CCCCCC", [(0, 5, 2), (0, 1, 1), (1, 2, 2), (2, 3, 1), (3, 4, 2), (4, 0, 1)], [0, 1, 1, 1, 1, 2]), {"alkene"}, set()),
        ("water", molecule("O", [], [2]), set(), set()),
        ("formamide", molecule("CNO", [(0, 1, 1), (0, 2, 2)], [1, 2, 0]), set(), set()),
        ("urea", molecule("CNNO", [(0, 1, 1), (0, 2, 1), (0, 3, 2)], [0, 2, 2, 0]), set(), set()),
        ("CO2", molecule("COO", [(0, 1, 2), (0, 2, 2)], [0, 0, 0]), set(), set()),
    ]
    return rows


def other_kekule_drawings():
    """{name: molecule}: the second Kekule drawing of four molecules of the table, atoms numbered as there."""
    benz = _ring(False)
    return {
        "benzene": molecule("CCCCCC", benz, [1] * 6),
        "toluene": molecule("CCCCCCC", benz + [(0, 6, 1)], [0, 1, 1, 1, 1, 1, 3]),
        "pyridine": molecule("NCCCCC", benz, [0, 1, 1, 1, 1, 1]),
        "naphthalene": molecule("C" * 10, _NAPHTHALENE[1], _NAPHTHALENE_H),
    }


def implicit_hydrogen_cases():
    """[(name in the table, the molecule with explicit hydrogens left out)]: the groups stay."""
    return [("ethanol", molecule("CCO", [(0, 1, 1), (1, 2, 1)], [3, 2, 0])), ("methane", molecule("C", [], [3])),
            ("benzene", molecule("CCCCCC", _ring(True), [0] * 6)), ("acetic acid", molecule("CCOO", [(0, 1, 1), (1, 2, 2), (1, 3, 1)], [0, 0, 0, 0]))]


def quaterphenyl_29():
    """29 heavy atoms and no explicit hydrogen: four benzene rings in a row (the Kekule orders drawn one way in rings 0 and 2, the other way
    in rings 1 and 3), carrying F, OH, NH2, CH3 and a second OH: arene, haloalkane, alcohol, amine, alkane."""
    elements, bonds = "", []
    for k in range(4):
        base = 6 * k
        elements += "C" * 6
        bonds += [(base + i, base + j, o) for i, j, o in _ring(k % 2 == 0)]
        if k:
            bonds.append((base - 3, base, 1))
    elements += "FONCO"
    bonds += [(1, 24, 1), (8, 25, 1), (14, 26, 1), (20, 27, 1), (22, 28, 1)]
    return molecule(elements, bonds, [0] * 29)


SUBSTITUENTS = ("F", "OH", "NH2", "CH3", "CHO")


def substituted(mol, h, group):
    """``mol`` with its hydrogen atom ``h`` replaced by ``group``; the new atoms are appended."""
    types, fc = [int(t) for t in mol["type"]], [int(c) for c in mol["fc"]]
    n = len(types)
    assert types[h] == H
    bonds = [(i, j, int(mol["bond"][i, j])) for i in range(n) for j in range(i + 1, n) if mol["bond"][i, j]]
    head, extra = {"F": (F, []), "OH": (O, [(H, 1)]), "NH2": (N, [(H, 1)] * 2), "CH3": (C, [(H, 1)] * 3), "CHO": (C, [(O, 2), (H, 1)])}[group]
    types[h] = head
    for t, order in extra:
        bonds.append((h, len(types), order))
        types.append(t)
        fc.append(0)
    return VM.molecule(types, bonds, fc=fc)


def derived_set(seed=20261020, plain=7, ringed=12):
    """About 300 molecules: every molecule of the table that has a hydrogen with one hydrogen (half of the time a second one) replaced by F /
    OH / NH2 / CH3 / CHO, ``plain`` times each; the four molecules with a non-aromatic ring ``ringed`` times, so that the set has enough of
    them.  Fixed by the seed."""
    rng = np.random.default_rng(seed)
    out = []
    for name, mol, groups, aromatic in hand_table():
        if not (np.asarray(mol["type"]) == H).any():
            continue
        for _ in range(ringed if name in ("cyclopentadiene", "4H-pyran", "p-benzoquinone", "fulvene") else plain):
            new = mol
            for _ in range(1 + int(rng.integers(2))):
                hs = np.nonzero(np.asarray(new["type"]) == H)[0]
                if hs.size == 0:                                               # HCN after F
                    break
                new =substituted(new, int(rng.choice(hs)), SUBSTITUENTS[int(rng.integers(len(SUBSTITUENTS)))])
            out.append(new)
    return out


def records_of(mols):
    """(rec [len, 1248] u8, n [len] i32) as numpy arrays through the project's ``records_from_graph``: the collated tensors of a processed file
    with the types as their own list, both directions of every bond in the edge list."""
    from diffspectra_amd.structure_metrics import records_from_graph
    counts = [len(m["type"]) for m in mols]
    edges = [[(i, j, int(m["bond"][i, j])) for i in range(k) for j in range(k) if i != j and m["bond"][i, j]] for m, k in zip(mols, counts)]
    flat = [e for es in edges for e in es]
    node_slices = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int64)
    edge_slices = torch.tensor(np.concatenate([[0], np.cumsum([len(es) for es in edges])]), dtype=torch.int64)
    rec = records_from_graph(torch.tensor(np.concatenate([m["type"] for m in mols]), dtype=torch.int64),
                             torch.tensor(np.concatenate([m["pos"] for m in mols]), dtype=torch.float32),
                             torch.tensor(np.concatenate([m["fc"] for m in mols]), dtype=torch.int64),
                             torch.tensor([[i for i, _, _ in flat], [j for _, j, _ in flat]], dtype=torch.int64).reshape(2, -1),
                             torch.tensor([o for _, _, o in flat], dtype=torch.int64), node_slices, edge_slices, atom_type_list=range(5))
    return rec.numpy(), np.asarray(counts, np.int32)
