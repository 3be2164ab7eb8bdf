"""CPU yardstick of ``dsk_scaffold_masks`` and of the Scaf arithmetic in plain Python, written from the text of include/diffspectra_scaffold.h and
not from the kernel: the heavy graph, the 2-core by deleting one atom at a time (the header says the order does not matter; the kernel deletes
a whole round at once), exocyclic atoms, ring bonds by a breadth-first search without the bond, components by a depth-first search, and the
cyclomatic ring count.  It works on raw record bytes, so whatever the contract says is ignored can hold garbage.  Scaffold identity is
``graph_mirror.same_graph`` on the mirror's own extraction (``valence_mirror.fragment`` with the scaffold mask).

Also here: the hand-stated table of molecules (the pin: RDKit cannot run where the project runs) and the seeded derived set that the CPU test
checks for coverage and the GPU test compares on.
"""
from __future__ import annotations

import math

import numpy as np

from tests import graph_mirror as GM, groups_mirror as G, structure_mirror as SM, valence_mirror as VM

OK, UNUSABLE = 0, 3
H, C, N, O, F = range(5)
KEYS = ("scaffold_mask", "ring_mask", "summary", "status")


def parts(rec, n):
    """The header's sets of one record, None for an unusable one: dict(heavy, core, exocyclic, ring, linker, rings), atoms as sets."""
    n, types, raw, orders, usable, _ = VM.read(rec, n, VM.RECORD)
    if not usable:
        return None
    heavy = {i for i in range(n) if 1 <= types[i] <= 4}
    nbrs = {i: {j for j in heavy if j != i and orders[i][j] > 0} for i in heavy}                # hydrogens and all their bonds are gone
    core = set(heavy)
    while True:                                                                                 # one deletion at a time, highest atom first
        loose = [i for i in sorted(core, reverse=True) if len(nbrs[i] & core) <= 1]
        if not loose:
            break
        core.discard(loose[0])
    exocyclic = {i for i in heavy - core if len(nbrs[i]) == 1 and nbrs[i] <= core and orders[i][next(iter(nbrs[i]))] >= 2}
    cnbrs = {i: nbrs[i] & core for i in core}

    def reaches(a, b):
        """b from a over core bonds without the bond a-b."""
        seen, queue = {a}, [a]
        while queue:
            u = queue.pop(0)
            for v in sorted(cnbrs[u]):
                if {u, v} == {a, b} or v in seen:
                    continue
                if v == b:
                    return True
                seen.add(v)
                queue.append(v)
        return False
    ring = {a for a in core if any(reaches(a, b) for b in cnbrs[a])}
    bonds = sum(len(cnbrs[i]) for i in core) // 2
    left, components = set(core), 0
    while left:
        components += 1
        stack = [left.pop()]
        while stack:
            u = stack.pop()
            for v in cnbrs[u] & left:
                left.discard(v)
                stack.append(v)
    return dict(heavy=heavy, core=core, exocyclic=exocyclic, ring=ring, linker=core - ring, rings=bonds - len(core) + components)


def analyse(rec, n):
    """One row of ``dsk_scaffold_masks``: dict(scaffold_mask, ring_mask, summary (4), status)."""
    p = parts(rec, n)
    if p is None:
        return dict(scaffold_mask=0, ring_mask=0, summary=(0, 0, 0, 0), status=UNUSABLE)
    scaffold = p["core"] | p["exocyclic"]
    return dict(scaffold_mask=VM.bits(scaffold), ring_mask=VM.bits(p["ring"]), summary=(len(p["heavy"]), len(scaffold), p["rings"], len(p["ring"])),
                status=OK)


def analyse_table(rec, n):
    return [analyse(r, k) for r, k in zip(np.asarray(rec), np.asarray(n))]


def has_scaffold(row, min_rings):
    return row["status"] == OK and row["scaffold_mask"] != 0 and row["summary"][2] >= min_rings


def scaffold_mol(rec, n, bond_orders=True, row=None):
    """The scaffold of one record as a molecule dict: its scaffold atoms in original order with the applied charges (the header of
    dsv_fragment_records); ``bond_orders=False`` sets every non-zero bond to 1."""
    row = analyse(rec, n) if row is None else row
    mol = SM.mol_from_record(*VM.fragment(rec, n, row["scaffold_mask"], VM.RECORD, True))
    if not bond_orders:
        mol["bond"] = np.minimum(mol["bond"], 1)
    return mol


def same_scaffold(a, b, min_rings=1, bond_orders=True):
    """The verdict of ``scaffold_identity_batch`` on two (rec, n) rows: (same, status)."""
    ra, rb = analyse(*a), analyse(*b)
    if ra["status"] != OK or rb["status"] != OK:
        return False, UNUSABLE
    ha, hb = has_scaffold(ra, min_rings), has_scaffold(rb, min_rings)
    if not ha or not hb:
        return ha == hb, OK
    return GM.same_graph(scaffold_mol(*a, bond_orders, ra), scaffold_mol(*b, bond_orders, rb)), OK


def unique_rows(rec, n):
    """The lowest row of every class of identical molecules (whole records, ``graph_mirror.same_graph``), ascending."""
    kept, mols = [], []
    for p, (r, k) in enumerate(zip(rec, n)):
        mol = SM.mol_from_record(r, k)
        if not any(GM.same_graph(mol, other) for other in mols):
            kept.append(p)
            mols.append(mol)
    return kept


def scaffold_counts(rec, n, min_rings, bond_orders=True, classes=None):
    """(classes, counts, class of every row or -1): ``classes`` is a list of scaffold molecules that is extended in place, so that two sides
    counted one after the other share their class numbers; ``counts[k]`` is this side's number of molecules with scaffold ``classes[k]``."""
    classes = [] if classes is None else classes
    counts, of_row = {}, []
    for r, k in zip(np.asarray(rec), np.asarray(n)):
        row = analyse(r, k)
        if not has_scaffold(row, min_rings):
            of_row.append(-1)
            continue
        mol = scaffold_mol(r, k, bond_orders, row)
        for c, other in enumerate(classes):
            if GM.same_graph(mol, other):
                break
        else:
            c = len(classes)
            classes.append(mol)
        counts[c] = counts.get(c, 0) + 1
        of_row.append(c)
    return classes, counts, of_row


def cosine(g, t):
    """Scaf of two count tables {scaffold: count}: exact integer sums, one division and one square root."""
    dot, gg, tt = sum(c * t[k] for k, c in g.items() if k in t), sum(c * c for c in g.values()), sum(c * c for c in t.values())
    return dot / math.sqrt(gg * tt) if gg and tt else float("nan")


def scaffold_metric(gen, test, min_rings=2, bond_orders=True):
    """What ``get_scaffold_metric(test, min_rings, unique=False, bond_orders)(gen)`` gives, the class ids as this mirror numbers them; ``gen``
    and ``test`` are (rec, n) pairs of arrays."""
    classes, t, _ = scaffold_counts(*test, min_rings, bond_orders)
    _, g, of_row = scaffold_counts(*gen, min_rings, bond_orders, classes)
    usable = [row for row in analyse_table(*gen) if row["status"] == OK]
    return dict(scaf=cosine(g, t), n_generated=len(gen[1]), n_test=len(test[1]), with_scaffold_generated=sum(g.values()), with_scaffold_test=sum(t.values()),
                distinct_generated=len(g), distinct_test=len(t), shared=len(set(g) & set(t)), scaffold_class=of_row,
                mean_rings=sum(row["summary"][2] for row in usable) / len(usable) if usable else float("nan"))


def scaf(gen_rows, test_rows, min_rings=2, bond_orders=True):
    return scaffold_metric(gen_rows, test_rows, min_rings, bond_orders)["scaf"]


# ------------------------------------------------------------------------------------------------------------------ molecules

def _cycle(*atoms, order=1):
    return [(a, b, order) for a, b in zip(atoms, atoms[1:] + atoms[:1])]


def hand_table():
    """[(name, molecule, scaffold atoms, ring atoms, rings)]: stated by hand from the header's definitions, not computed.  The heavy atoms
    come first in every molecule, so stripping the hydrogens keeps their numbers."""
    mol = G.molecule
    three, six = {0, 1, 2}, set(range(6))
    two_rings = _cycle(0, 1, 2) + _cycle(3, 4, 5)
    bridged = VM.molecule([C] * 6 + [H] * 11, two_rings + [(0, 6, 1), (3, 6, 1)] + [(a, 7 + k, 1) for k, a in enumerate((0, 1, 1, 2, 2, 3, 4, 4, 5, 5))])
    return [
        ("hexane", mol("CCCCCC", [(i, i + 1, 1) for i in range(5)], [3, 2, 2, 2, 2, 3]), set(), set(), 0),
        ("methane", mol("C", [], [4]), set(), set(), 0),
        ("water", mol("O", [], [2]), set(), set(), 0),
        ("cyclohexane", mol("CCCCCC", _cycle(*range(6)), [2] * 6), six, six, 1),
        ("toluene", mol("CCCCCCC", G._ring(True) + [(0, 6, 1)], [0, 1, 1, 1, 1, 1, 3]), six, six, 1),
        ("cyclohexanone", mol("CCCCCCO", _cycle(*range(6)) + [(0, 6, 2)], [0, 2, 2, 2, 2, 2, 0]), six | {6}, six, 1),
        ("methylenecyclopropane", mol("CCCC", _cycle(0, 1, 2) + [(0, 3, 2)], [0, 2, 2, 2]), three | {3}, three, 1),
        ("1-cyclohexylethanone", mol("CCCCCCCOC", _cycle(*range(6)) + [(0, 6, 1), (6, 7, 2), (6, 8, 1)], [1, 2, 2, 2, 2, 2, 0, 0, 3]), six, six, 1),
        ("cyclopropanol", mol("CCCO", _cycle(0, 1, 2) + [(0, 3, 1)], [1, 2, 2, 1]), three, three, 1),
        ("cyclopropyl-CH=NH", mol("CCCCN", _cycle(0, 1, 2) + [(0, 3, 1), (3, 4, 2)], [1, 2, 2, 1, 1]), three, three, 1),
        ("dicyclopropyl ketone", mol("CCCCCCCO", two_rings + [(0, 6, 1), (3, 6, 1), (6, 7, 2)], [1, 2, 2, 1, 2, 2, 0, 0]), set(range(8)), six, 2),
        ("1,2-dicyclopropylpropane", mol("CCCCCCCCC", two_rings + [(0, 6, 1), (6, 7, 1), (7, 3, 1), (7, 8, 1)], [1, 2, 2, 1, 2, 2, 2, 1, 3]),
         set(range(8)), six, 2),
        ("spiropentane", mol("CCCCC", _cycle(0, 1, 2) + _cycle(0, 3, 4), [0, 2, 2, 2, 2]), set(range(5)), set(range(5)), 2),
        ("bicyclo[1.1.0]butane", mol("CCCC", _cycle(0, 1, 2, 3) + [(0, 2, 1)], [1, 2, 1, 2]), set(range(4)), set(range(4)), 2),
        ("cubane", mol("C" * 8, [(i, i ^ b, 1) for i in range(8) for b in (1, 2, 4) if i < i ^ b], [1] * 8), set(range(8)), set(range(8)), 5),
        ("cyclopropane and cyclobutane", mol("C" * 7, _cycle(0, 1, 2) + _cycle(3, 4, 5, 6), [2] * 7), set(range(7)), set(range(7)), 2),
        ("two cyclopropanes bridged by a hydrogen", bridged, six, six, 2),
        ("1-methylaziridinium (ring N+)", mol("NCCC", _cycle(0, 1, 2) + [(0, 3, 1)], [1, 2, 2, 3], fc=[1, 0, 0, 0]), three, three, 1),
        ("pyridine N-oxide (N+, O-)", mol("NCCCCCO", G._ring(True) + [(0, 6, 1)], [0, 1, 1, 1, 1, 1, 0], fc=[1, 0, 0, 0, 0, 0, -1]), six, six, 1),
    ]


def stripped(mol):
    """The molecule without its hydrogens (the implicit-hydrogen form); the heavy atoms keep their order."""
    keep = np.nonzero(np.asarray(mol["type"]) != H)[0]
    return dict(pos=mol["pos"][keep], type=mol["type"][keep].copy(), fc=mol["fc"][keep].copy(), bond=mol["bond"][np.ix_(keep, keep)].copy())


def other_kekule_toluene():
    """The second Kekule drawing of the table's toluene, atoms numbered as there."""
    return G.molecule("CCCCCCC", G._ring(False) + [(0, 6, 1)], [0, 1, 1, 1, 1, 1, 3])


def kekule_pair():
    """The two Kekule drawings of 2-cyclopropylpyridine (N 0, ring carbons 1..5, the cyclopropyl 6..8 on carbon 1), atoms numbered alike: N=C(R)
    in the first, N-C(R)= in the second.  No symmetry of the scaffold maps one drawing onto the other, so they are two labelled graphs -
    unlike the drawings of toluene, which are mirror images of each other (atom 1 <-> atom 5) and so one graph."""
    tail = [(1, 6, 1)] + _cycle(6, 7, 8)
    hydrogens = [0, 0, 1, 1, 1, 1, 1, 2, 2]
    return G.molecule("NCCCCCCCC", G._ring(True) + tail, hydrogens), G.molecule("NCCCCCCCC", G._ring(False) + tail, hydrogens)


def named(name):
    return [mol for nm, mol, _, _, _ in hand_table() if nm == name][0]


def hand_pairs():
    """[(name, molecule, molecule, same scaffold at min_rings = 1)], stated by hand."""
    mol = G.molecule
    butane = mol("CCCC", [(i, i + 1, 1) for i in range(3)], [3, 2, 2, 3])
    ethylbenzene = mol("CCCCCCCC", G._ring(True) + [(0, 6, 1), (6, 7, 1)], [0, 1, 1, 1, 1, 1, 2, 3])
    cyclohexanol = mol("CCCCCCO", _cycle(*range(6)) + [(0, 6, 1)], [1, 2, 2, 2, 2, 2, 1])
    return [("hexane / butane", named("hexane"), butane, True), ("toluene / hexane", named("toluene"), named("hexane"), False),
            ("toluene / ethylbenzene", named("toluene"), ethylbenzene, True), ("cyclohexanone / cyclohexanol", named("cyclohexanone"), cyclohexanol, False)]


def derived_set(seed=20261020, grown=10, trees=45, closed=70):
    """About 300 molecules, fixed by the seed: every molecule of the table with one hydrogen (half of the time a second one) replaced by a
    substituent of ``groups_mirror.substituted`` while the molecule still fits a record, ``grown`` times each; ``trees`` tree molecules of
    ``structure_mirror.random_tree_molecule`` (no scaffold); ``closed`` molecules of ``graph_mirror.random_molecule`` (0-3 ring closures), every other one with its hydrogens
    turned into carbons."""
    rng = np.random.default_rng(seed)
    out = []
    for name, mol, _, _, _ in hand_table():
        for _ in range(grown):
            new = mol
            for _ in range(1 + int(rng.integers(2))):
                hs = np.nonzero((np.asarray(new["type"]) == H) & ((np.asarray(new["bond"]) > 0).sum(1) == 1))[0]       # not the bridging hydrogen
                group = G.SUBSTITUENTS[int(rng.integers(len(G.SUBSTITUENTS)))]
                if hs.size == 0:
                    break
                grown_mol = G.substituted(new, int(rng.choice(hs)), group)
                if len(grown_mol["type"]) <= SM.W:
                    new = grown_mol
            out.append(new)
    for _ in range(trees):
        pos, types, fc, bond = SM.random_tree_molecule(rng, int(rng.integers(3, 20)))
        out.append(dict(pos=pos, type=types, fc=fc, bond=bond))
    for k in range(closed):
        mol = GM.random_molecule(rng, int(rng.integers(6, 24)))
        if k % 2:                                                              # half of the atoms there are hydrogens, and a closure through one
            mol["type"] = np.where(mol["type"] == H, C, mol["type"])           # closes no ring: every other molecule gets carbons instead
        out.append(mol)
    return out
