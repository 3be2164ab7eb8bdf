"""CPU yardstick of ``dsq_match_records`` in plain Python, written from the text of include/diffspectra_substructure.h and not from the kernel: the
hydrogen-folded matched graph, the per-atom property word, the eight bond classes (aromatic bonds as consecutive atoms of an aromatic cycle),
and the header's depth-first search with its node count, truncated results included.  The per-atom quantities, the ring-bond test and the
electron rule are those of tests/groups_mirror.py (the header refers to diffspectra_groups.h for them).  It reads the packed pattern words, so it
checks the parser's packing too, and works on raw record bytes, so whatever the contract says is ignored can hold garbage.

Also here: the MACCS evaluation on top of the matcher (``maccs_row``) and the hand-stated table of molecules with their MACCS sets.
"""
from __future__ import annotations

import numpy as np

from diffspectra_amd import maccs, smarts
from tests import groups_mirror as G, valence_mirror as VM

OK, UNUSABLE, INVALID = 0, 2, 3
COUNT_CAP, TRUNCATED = 4, 128
MAX_ATOMS, MAX_CLOSURES = 14, 2
DEFAULT_NODES = 1 << 18
H = 0


class Graph:
    """One record as the header sees it."""

    def __init__(self, rec, n):
        n, types, raw, orders, usable, _ = VM.read(rec, n, VM.RECORD)
        self.usable = usable
        if not usable:
            return
        self.n = n
        atoms = [G.Atom(i, types, raw, orders) for i in range(n)]
        folded = [A.t == H and raw[A.i] == 0 and A.D == 1 and orders[A.i][A.nbrs[0]] == 1 and types[A.nbrs[0]] != H for A in atoms]
        self.matchable = [i for i in range(n) if not folded[i]]
        ring = {(a, b): G.ring_bond(atoms, a, b) for a in range(n) for b in atoms[a].nbrs}
        cycles = aromatic_cycles(atoms)
        self.aromatic = sorted({i for path in cycles for i in path})
        self.aromatic_rings = min(4, len({frozenset(path) for path in cycles}))
        aromatic_bonds = {frozenset((path[k], path[(k + 1) % len(path)])) for path in cycles for k in range(len(path))}
        self.cls = {}                                                          # (a, b) -> class of the bond, both ways, matchable atoms only
        for a in self.matchable:
            for b in atoms[a].nbrs:
                if not folded[b]:
                    kind = 3 if frozenset((a, b)) in aromatic_bonds else orders[a][b] - 1
                    self.cls[a, b] = kind + 4 * int(ring[a, b])
        self.props = {}
        for a in self.matchable:
            A = atoms[a]
            D = sum(1 for b in A.nbrs if not folded[b])
            on_ring = any(ring[a, b] for b in A.nbrs)
            self.props[a] = (1 << (2 * A.t + int(a in self.aromatic))) | (1 << (10 + min(A.Ht, 4))) | (1 << (15 + min(A.X, 4))) | (1 << (20 + min(D, 4))) | \
                (1 << (25 + int(on_ring))) | (1 << (27 + A.q + 1))
        self.fragments = len(VM.components(n, orders))                         # a folded hydrogen hangs on a matchable atom: the same number

    def satisfies(self, a, word):
        return bin(word & self.props[a]).count("1") == 6

    def bonded(self, a, b, allowed):
        c = self.cls.get((a, b))
        return c is not None and (allowed >> c) & 1 == 1


def aromatic_cycles(atoms):
    """Every aromatic cycle (a simple cycle of 5 or 6 atoms that passes the electron rule) as a path from its lowest atom, in both directions."""
    walk = [not G.never_candidate(A) for A in atoms]
    found = []

    def extend(path):
        last = atoms[path[-1]]
        if len(path) in (5, 6) and path[0] in last.nbrs:
            counts = [G.electrons(atoms, atoms[i], set(path)) for i in path]
            if None not in counts and sum(counts) == 6:
                found.append(list(path))
        if len(path) < 6:
            for v in last.nbrs:
                if v > path[0] and walk[v] and v not in path:
                    extend(path + [v])
    for s in range(len(atoms)):
        if walk[s]:
            extend([s])
    return found


def well_formed(w):
    A, C = w[0] & 255, (w[0] >> 8) & 255
    if not 1 <= A <= MAX_ATOMS or C > MAX_CLOSURES:
        return False
    if any((w[15 + k] & 255) >= k for k in range(1, A)):
        return False
    return all((w[29 + c] & 255) < ((w[29 + c] >> 8) & 255) < A for c in range(C))


def match(g: Graph, words, max_nodes=DEFAULT_NODES):
    """One entry of the kernel's [P, K] outputs: dict(count (with the TRUNCATED bit), anchors, cover)."""
    w = [int(x) & 0xFFFFFFFF for x in words]
    if not g.usable or not well_formed(w):
        return dict(count=0, anchors=0, cover=0)
    A, C = w[0] & 255, (w[0] >> 8) & 255
    closures = [(w[29 + c] & 255, (w[29 + c] >> 8) & 255, (w[29 + c] >> 16) & 255) for c in range(C)]
    sets, anchors, cover, truncated = set(), 0, 0, False

    def record(image):
        nonlocal anchors, cover
        mask = VM.bits(image)
        sets.add(mask)
        anchors |= 1 << image[0]
        cover |= mask

    for start in g.matchable:
        if not g.satisfies(start, w[1]):
            continue
        if A == 1:
            record([start])
            continue
        image, nodes = [start], 0

        def assign(k):
            """False once the search has stopped."""
            nonlocal nodes
            parent, allowed = w[15 + k] & 255, (w[15 + k] >> 8) & 255
            for c in g.matchable:                                              # ascending record index
                if c in image or not g.satisfies(c, w[1 + k]) or not g.bonded(image[parent], c, allowed):
                    continue
                if not all(g.bonded(image[a], c, s) for a, b, s in closures if b == k):
                    continue
                nodes += 1
                if k == A - 1:
                    record(image + [c])
                if nodes >= max_nodes:
                    return False
                if k < A - 1:
                    image.append(c)
                    more = assign(k + 1)
                    image.pop()
                    if not more:
                        return False
            return True
        if not assign(1):
            truncated = True
    return dict(count=min(len(sets), COUNT_CAP) | (TRUNCATED if truncated else 0), anchors=anchors, cover=cover)


def analyse(rec, n, patterns, max_nodes=DEFAULT_NODES):
    """One row of ``dsq_match_records``: dict(count [K], anchors [K], cover [K], aromatic_mask, aromatic_rings, fragments, status)."""
    g = Graph(rec, n)
    K = len(patterns)
    if not g.usable:
        return dict(count=[0] * K, anchors=[0] * K, cover=[0] * K, aromatic_mask=0, aromatic_rings=0, fragments=0, status=UNUSABLE)
    rows = [match(g, p, max_nodes) for p in patterns]
    return dict(count=[r["count"] for r in rows], anchors=[r["anchors"] for r in rows], cover=[r["cover"] for r in rows],
                aromatic_mask=VM.bits(g.aromatic), aromatic_rings=g.aromatic_rings, fragments=g.fragments, status=OK)


def analyse_table(rec, n, patterns, max_nodes=DEFAULT_NODES):
    return [analyse(r, k, patterns, max_nodes) for r, k in zip(np.asarray(rec), np.asarray(n))]


def as_arrays(rows, K):
    """The rows of ``analyse_table`` as the seven arrays of the kernel."""
    P = len(rows)
    i32 = lambda key: np.array([r[key] for r in rows], np.int64).astype(np.int32).reshape(P)
    return (np.array([r["count"] for r in rows], np.uint8).reshape(P, K), np.array([r["anchors"] for r in rows], np.int64).astype(np.int32).reshape(P, K),
            np.array([r["cover"] for r in rows], np.int64).astype(np.int32).reshape(P, K), i32("aromatic_mask"), i32("aromatic_rings"), i32("fragments"),
            np.array([r["status"] for r in rows], np.uint8))


# ------------------------------------------------------------------------------------------------------------------ MACCS

MACCS_TEXTS, MACCS_SINGLE, MACCS_ANCHORED = maccs.pattern_table()
MACCS_WORDS = smarts.compile_patterns(MACCS_TEXTS)


def maccs_of(row):
    """(set of the keys a row of ``analyse`` over ``MACCS_WORDS`` sets, any entry truncated), from ``maccs.MACCS_KEYS`` itself."""
    column = {text: c for c, text in enumerate(MACCS_TEXTS)}
    keys = set()
    for key, (name, alternatives, threshold) in enumerate(maccs.MACCS_KEYS, start=1):
        if key == 125:
            hit = row["aromatic_rings"] > 1
        elif key == 166:
            hit = row["fragments"] > 1
        elif alternatives is None:
            hit = False
        elif key in maccs._ANCHORED:
            atoms = 0
            for text in alternatives:
                atoms |= row["anchors"][column[text]]
            hit = bin(atoms).count("1") > threshold
        else:
            hit = (row["count"][column[alternatives[0]]] & (TRUNCATED - 1)) > threshold
        if hit:
            keys.add(key)
    return keys, any(c & TRUNCATED for c in row["count"])


def maccs_row(rec, n, max_nodes=DEFAULT_NODES):
    row = analyse(rec, n, MACCS_WORDS, max_nodes)
    keys, truncated = maccs_of(row)
    return dict(keys=keys, truncated=truncated, status=row["status"])


def tanimoto(a: set, b: set):
    return 1.0 if not (a | b) else len(a & b) / len(a | b)


# ------------------------------------------------------------------------------------------------------------------ molecules

def _cycloalkane(size):
    return G.molecule("C" * size, [(i, (i + 1) % size, 1) for i in range(size)], [2] * size)


def _biphenyl():
    bonds = G._ring(True) + [(6 + i, 6 + j, o) for i, j, o in G._ring(False)] + [(0, 6, 1)]
    return G.molecule("C" * 12, bonds, [0, 1, 1, 1, 1, 1] * 2)


def _fluorene():
    """Ring A = atoms 0..5, ring B = atoms 6..11, the five-ring 0, 5, 12 (CH2), 6, 11... drawn as: A fused at 0-5, B fused at 6-11, the single
    bond 0-6 and the bridge 5-12-11."""
    bonds = G._ring(True) + [(6 + i, 6 + j, o) for i, j, o in G._ring(True)] + [(0, 6, 1), (5, 12, 1), (12, 11, 1)]
    return G.molecule("C" * 13, bonds, [0, 1, 1, 1, 1, 0, 0, 1, 1, 1, 1, 0, 2])


def maccs_table():
    """[(name, molecule, MACCS keys expected)].  The first five sets are the issue's; every other was derived by hand from the key table of
    diffspectra_amd/maccs.py and the header's definitions, key by key, and is stated here - not computed."""
    by_name = {name: mol for name, mol, _, _ in G.hand_table()}
    return [
        ("ethanol", by_name["ethanol"], {82, 109, 114, 139, 153, 155, 157, 160, 164}),
        ("benzene", by_name["benzene"], {162, 163, 165}),
        ("acetic acid", by_name["acetic acid"], {123, 139, 154, 157, 159, 160, 164}),
        ("pyridine", by_name["pyridine"], {65, 98, 121, 137, 161, 162, 163, 165}),
        ("methane", by_name["methane"], {160}),
        # one oxygen with hydrogens: [O;!H0] and [#8]
        ("water", by_name["water"], {139, 164}),
        # two CH2 joined by a double bond: [CH2]=* and [#6]=[#6]
        ("ethene", by_name["ethene"], {34, 99}),
        ("ethyne", by_name["ethyne"], {17}),
        # F, a halogen, on a CH3 that is [C;H3,H4] and has a hetero neighbour
        ("fluoromethane", by_name["fluoromethane"], {42, 93, 134, 160}),
        # NH2 (84, 151, 161) single-bonded (158) to a CH3 (160) that has a hetero neighbour (93)
        ("methylamine", by_name["methylamine"], {84, 93, 151, 158, 160, 161}),
        ("formaldehyde", G.molecule("CO", [(0, 1, 2)], [2, 0]), {34, 154, 164}),
        # three-ring (22); CH2-CH2 closes through the third atom, so the ring alternatives of 118 and 147 anchor on all three atoms
        ("cyclopropane", _cycloalkane(3), {22, 118, 147, 165}),
        # four-ring (11); *~[CH2]~[CH2]~* is a path of four atoms round the ring
        ("cyclobutane", _cycloalkane(4), {11, 118, 147, 165}),
        # eight-ring (101); paths of six and seven atoms with CH2 in second and second-last place (129, 128)
        ("cyclooctane", _cycloalkane(8), {101, 118, 128, 129, 147, 165}),
        ("cyclononane", _cycloalkane(9), {101, 118, 128, 129, 147, 165}),
        # O-C-C-O (72, 54 with both OH), C~CH2~OH (82, 109, 104, 132), O~CH2~C twice (153, 138), CH2-CH2 anchored at both O (118, 147), two OH (131,
        # 139, 159, 164), chain CH2 (155), C-O (157)
        ("ethylene glycol", G.molecule("OCCO", [(0, 1, 1), (1, 2, 1), (2, 3, 1)], [1, 2, 2, 1]),
         {54, 72, 82, 104, 109, 118, 131, 132, 138, 139, 147, 153, 155, 157, 159, 164}),
        # +H3N-CH2-COO-: charges (49), NH3+ is [#7;!H0] but not [NH2], N~CH2~C (82, 100, 153, 155), N-C (158), N~C~C~O (95), O~C~CH2~N (132),
        # O~C~O (123), C=O (154), C-O (157), two O (159, 164), N (161); no O carries a hydrogen
        ("glycine zwitterion", G.molecule("NCCOO", [(0, 1, 1), (1, 2, 1), (2, 3, 2), (2, 4, 1)], [3, 2, 0, 0, 0], fc=[1, 0, 0, 0, -1]),
         {49, 82, 95, 100, 123, 132, 151, 153, 154, 155, 157, 158, 159, 161, 164}),
        ("methane and water", G.molecule("CO", [], [4, 2]), {139, 160, 164, 166}),
        # two aromatic six-rings (125, 145, 162, 163), fusion atoms with three ring bonds (105), the ten-atom perimeter (101)
        ("naphthalene", by_name["naphthalene"], {101, 105, 125, 145, 162, 163, 165}),
        # two aromatic six-rings joined by a single chain bond between ring atoms (62); no atom has three ring bonds, no large cycle
        ("biphenyl", _biphenyl(), {62, 125, 145, 162, 163, 165}),
        # the five-ring (96) has three non-aromatic bonds: CH2 ~ c : c - c gives 144; fusion atoms (105); cycles of 9 and 13 atoms (101)
        ("fluorene", _fluorene(), {96, 101, 105, 125, 144, 145, 162, 163, 165}),
    ]


def oxygen_cases():
    """Molecules with three, four and five oxygens for the saturating count and key 140 ([#8] > 3)."""
    three = G.molecule("COOO", [(0, 1, 1), (0, 2, 1), (0, 3, 1)], [1, 1, 1, 1])
    four = G.molecule("COOOO", [(0, 1, 1), (0, 2, 1), (0, 3, 1), (0, 4, 1)], [0, 1, 1, 1, 1])
    five = G.molecule("CCOOOOO", [(0, 1, 1), (0, 2, 1), (0, 3, 1), (0, 4, 1), (1, 5, 1), (1, 6, 1)], [0, 1, 1, 1, 1, 1, 1])
    return three, four, five
