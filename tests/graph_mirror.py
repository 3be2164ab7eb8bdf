"""CPU yardstick of ``ds_graph_identity_records`` and ``ds_graph_hash_records`` (include/diffspectra_hip.h), in plain Python.

``same_graph`` decides whether two molecules are the same labelled graph (atom type, formal charge, bond order) by a textbook
backtracking search: atoms of the first molecule are taken in a connected order and every one is tried on every unused atom of the second
with the same type, charge and degree whose bonds to the atoms mapped so far agree.  It shares nothing with the kernel's method (joint colour
refinement with individualisation), so an agreement of the two is evidence for both.  ``graph_hash`` restates the hash formula of the
header with Python integers.  A molecule is the dict of ``structure_mirror.mol_from_record`` (``type [n], fc [n], bond [n,n]``; ``pos`` is
never read).  No networkx: the GPU machine may not have it (tests/test_graph_identity_cpu.py checks this module against it where it exists).

Also here: the hard pairs (graphs that colour refinement cannot tell apart) and the seeded pair set that the parity test, the networkx
cross-check and tools/graph_bench.py share.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import structure_mirror as SM

W = SM.W
MASK = (1 << 64) - 1


def _adjacency(mol):
    """Bond bytes as a symmetric list of lists: the upper triangle of the record's matrix decides, the diagonal is no pair."""
    n = len(mol["type"])
    b = np.asarray(mol["bond"]).astype(np.int64) & 255
    up = np.triu(b[:n, :n], 1)
    return (up + up.T).tolist()


def same_graph(a, b, want_map=False):
    """True when a bijection of the atoms preserves type, charge byte and the bond byte of every pair (whole molecules).  ``want_map=True``
    returns ``(answer, map or None)`` with ``map[i]`` the atom of ``b`` that atom ``i`` of ``a`` goes to."""
    n = len(a["type"])
    if n != len(b["type"]):
        return (False, None) if want_map else False
    A, B = _adjacency(a), _adjacency(b)
    lab = lambda m, adj: [(int(m["type"][i]), int(m["fc"][i]) & 255, sum(1 for x in adj[i] if x)) for i in range(n)]
    la, lb = lab(a, A), lab(b, B)
    if sorted(la) != sorted(lb):
        return (False, None) if want_map else False
    order, seen = [], [False] * n                    # a connected order: breadth first, the next piece starts at its lowest atom
    for s in range(n):
        if seen[s]:
            continue
        seen[s] = True
        queue = [s]
        while queue:
            v = queue.pop(0)
            order.append(v)
            for u in range(n):
                if A[v][u] and not seen[u]:
                    seen[u] = True
                    queue.append(u)
    image, used = [-1] * n, [False] * n

    def place(k):
        if k == n:
            return True
        v = order[k]
        for w in range(n):
            if used[w] or la[v] != lb[w]:
                continue
            if all(A[v][order[q]] == B[w][image[order[q]]] for q in range(k)):
                image[v], used[w] = w, True
                if place(k + 1):
                    return True
                image[v], used[w] = -1, False
        return False

    ok = place(0)
    return (ok, list(image) if ok else None) if want_map else ok


def is_isomorphism(a, b, image):
    """The check a test runs on a map the kernel returned: a bijection that preserves every type, charge byte and bond byte."""
    n = len(a["type"])
    image = [int(x) for x in image[:n]]
    if len(b["type"]) != n or sorted(image) != list(range(n)):
        return False
    A, B = _adjacency(a), _adjacency(b)
    return all(int(a["type"][i]) == int(b["type"][image[i]]) and (int(a["fc"][i]) & 255) == (int(b["fc"][image[i]]) & 255) for i in range(n)) and \
        all(A[i][j] == B[image[i]][image[j]] for i in range(n) for j in range(n))


# ------------------------------------------------------------------------------------------------------------------ the hash, restated

def fmix(x):
    x &= MASK
    x ^= x >> 30
    x = (x * 0xbf58476d1ce4e5b9) & MASK
    x ^= x >> 27
    x = (x * 0x94d049bb133111eb) & MASK
    return x ^ (x >> 31)


def mix(a, b):
    return fmix(a + 0x9e3779b97f4a7c15 * (b + 1))


def graph_hash(mol):
    """``ds_graph_hash_records`` of one molecule, from the formula in the header (unsigned 64-bit, wrap-around)."""
    n = len(mol["type"])
    A = _adjacency(mol)
    h = [mix(int(mol["type"][i]) & 255, int(mol["fc"][i]) & 255) for i in range(n)]
    for _ in range(W):
        h = [mix(h[i], sum(mix(h[j], A[i][j]) for j in range(n) if j != i and A[i][j] > 0) & MASK) for i in range(n)]
    return mix(n, sum(fmix(x) for x in h) & MASK)


# ------------------------------------------------------------------------------------------------------------------ molecules

def molecule(types, edges, fc=None, orders=None):
    """Molecule dict from an edge list (bond order 1 unless ``orders`` says otherwise)."""
    n = len(types)
    bond = np.zeros((n, n), np.int64)
    for k, (i, j) in enumerate(edges):
        bond[i, j] = bond[j, i] = 1 if orders is None else orders[k]
    return dict(pos=np.zeros((n, 3)), type=np.asarray(types, np.int64), fc=np.zeros(n, np.int64) if fc is None else np.asarray(fc, np.int64), bond=bond)


def carbons(n, edges):
    return molecule([1] * n, edges)


def k29():
    """The complete graph on 29 carbons: every class of the refinement is all of the molecule."""
    return carbons(29, [(i, j) for i in range(29) for j in range(i + 1, 29)])


def saturated(mol):
    """Hydrogens (type 0) on every atom up to valence 4."""
    n = len(mol["type"])
    types, edges = list(mol["type"]), [(i, j) for i in range(n) for j in range(i + 1, n) if mol["bond"][i, j]]
    for i in range(n):
        for _ in range(4 - int((mol["bond"][i] > 0).sum())):
            edges.append((i, len(types)))
            types.append(0)
    return molecule(types, edges)


def permuted(mol, rng):
    """The same graph with its atoms renamed and fresh, unrelated coordinates: new atom i is old atom perm[i]."""
    n = len(mol["type"])
    perm = rng.permutation(n)
    return dict(pos=rng.normal(size=(n, 3)) * 2.0, type=mol["type"][perm].copy(), fc=mol["fc"][perm].copy(), bond=mol["bond"][np.ix_(perm, perm)].copy())


def _path(*atoms):
    return list(zip(atoms[:-1], atoms[1:]))


def hard_pairs():
    """[(name, molecule, molecule)]: all-carbon graphs of equal degree sequence that colour refinement cannot separate, bare and saturated."""
    bare = [
        ("hexagon / two triangles", carbons(6, _path(0, 1, 2, 3, 4, 5, 0)), carbons(6, _path(0, 1, 2, 0) + _path(3, 4, 5, 3))),
        ("prism / K3,3", carbons(6, _path(0, 1, 2, 0) + _path(3, 4, 5, 3) + [(0, 3), (1, 4), (2, 5)]),
         carbons(6, [(i, j) for i in range(3) for j in range(3, 6)])),
        ("decalin / bicyclopentyl", carbons(10, _path(0, 1, 2, 3, 4, 5, 0) + _path(4, 6, 7, 8, 9, 5)),
         carbons(10, _path(0, 1, 2, 3, 4, 0) + _path(5, 6, 7, 8, 9, 5) + [(0, 5)])),
        ("cube / cuneane", carbons(8, [(i, i ^ b) for i in range(8) for b in (1, 2, 4) if i < i ^ b]),
         carbons(8, _path(0, 1, 2, 0) + _path(3, 4, 5, 6, 3) + [(0, 3), (1, 4), (2, 7), (7, 5), (7, 6)])),
    ]
    return bare + [(name + " (saturated)", saturated(a), saturated(b)) for name, a, b in bare]


def nonane():
    """A saturated C9H20 (2,2,4,4-tetramethylpentane: many equivalent hydrogens), 29 atoms."""
    return saturated(carbons(9, _path(0, 1, 2, 3, 4) + [(1, 5), (1, 6), (3, 7), (3, 8)]))


# ------------------------------------------------------------------------------------------------------------------ the seeded pair set

def random_molecule(rng, n):
    """A tree of ``structure_mirror.random_tree_molecule`` plus 0-3 ring-closing bonds between atoms of degree below 4."""
    pos, types, fc, bond = SM.random_tree_molecule(rng, n)
    for _ in range(int(rng.integers(0, 4))):
        deg = (bond > 0).sum(1)
        free = [(i, j) for i in range(n) for j in range(i + 1, n) if bond[i, j] == 0 and deg[i] < 4 and deg[j] < 4]
        if not free:
            break
        i, j = free[int(rng.integers(len(free)))]
        bond[i, j] = bond[j, i] = int(rng.choice([1, 1, 2]))
    return dict(pos=pos, type=types, fc=fc, bond=bond)


def _bond_switch(mol, rng):
    """a-b, c-d -> a-d, c-b on four distinct atoms with a-d and c-b unbonded: every atom keeps its degree and its bond orders."""
    bond = mol["bond"]
    n = len(bond)
    edges = [(i, j) for i in range(n) for j in range(n) if i != j and bond[i, j] > 0]              # directed: both orientations of a bond
    for _ in range(64):
        (a, b), (c, d) = edges[int(rng.integers(len(edges)))], edges[int(rng.integers(len(edges)))]
        if len({a, b, c, d}) == 4 and bond[a, d] == 0 and bond[c, b] == 0:
            ab, cd = bond[a, b], bond[c, d]
            bond[a, b] = bond[b, a] = bond[c, d] = bond[d, c] = 0
            bond[a, d] = bond[d, a] = ab
            bond[c, b] = bond[b, c] = cd
            return


def treated(mol, kind, rng):
    """The generated side of a pair: a permuted copy of ``mol`` with fresh coordinates after treatment ``kind``: 0 nothing more, 1 a
    degree-preserving bond switch, 2 one bond order changed, 3 the types of two atoms swapped."""
    m = dict(pos=mol["pos"], type=mol["type"].copy(), fc=mol["fc"].copy(), bond=mol["bond"].copy())
    n = len(m["type"])
    if kind == 1:
        _bond_switch(m, rng)
    elif kind == 2:
        i, j = np.argwhere(np.triu(m["bond"]) > 0)[int(rng.integers(int((np.triu(m["bond"]) > 0).sum())))]
        m["bond"][i, j] = m["bond"][j, i] = m["bond"][i, j] % 3 + 1
    elif kind == 3:
        i, j = rng.permutation(n)[:2]
        m["type"][i], m["type"][j] = m["type"][j], m["type"][i]
    return permuted(m, rng)


@functools.lru_cache(maxsize=4)
def seeded_pairs(count=2000, seed=20261018, sizes=None, kinds=(0, 1, 2, 3)):
    """(ref molecules, generated molecules, kind [count]): ground truths of 3-29 atoms (or of ``sizes``, a tuple) from ``random_molecule``, the
    generated side ``treated`` with ``kinds[p % len(kinds)]``.  What a pair's answer is decides ``same_graph``, not the recipe."""
    rng = np.random.default_rng(seed)
    ref, prb, kind = [], [], []
    for p in range(count):
        mol = random_molecule(rng, int(sizes[p]) if sizes is not None else int(rng.integers(3, W + 1)))
        ref.append(mol)
        kind.append(kinds[p % len(kinds)])
        prb.append(treated(mol, kind[-1], rng))
    return ref, prb, np.array(kind)


@functools.lru_cache(maxsize=4)
def seeded_labels(count=2000, seed=20261018):
    ref, prb, _ = seeded_pairs(count, seed)
    return np.array([same_graph(a, b) for a, b in zip(prb, ref)])
