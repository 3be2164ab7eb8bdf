"""CPU yardstick of ``ds_mces_records`` (include/diffspectra_hip.h): the maximum-common-edge-subgraph distance of two labelled molecular graphs.

    dist = W_A + W_B - 2 max_pi score(pi),    score(pi) = sum over bonds (i, j) of A with both ends mapped and (pi i, pi j) bonded in B of
                                                          min(w_A(i, j), w_B(pi i, pi j))

over partial injective maps pi that keep the atom type; W is a side's total bond weight, a weight is the bond-order byte, the formal charge
is not compared, and with ``drop_h`` the atoms of decoder type 0 and their bonds are left out first.

Two methods that share nothing with the kernel's branch-and-bound, and nothing with each other:

* ``mces_milp``: the integer program of ``myopic_mces`` restated on ``scipy.optimize.milp`` - binaries y[i, k] for same-type atom pairs and
  c[e, f] for type-compatible bond pairs, every atom and every bond used at most once per side, c[e, f] <= y[i, k] + y[i, l] and
  c[e, f] <= y[j, k] + y[j, l] for e = (i, j), f = (k, l), maximise sum c min(w).
* ``mces_exhaustive``: every partial injective type-preserving map, enumerated (usable up to about 6 kept atoms).

A molecule is the dict of ``structure_mirror.mol_from_record`` (``type [n], fc [n], bond [n, n]``; ``pos`` and ``fc`` are never read; bond
bytes come from the upper triangle).  Also here: the seeded pair set of the parity tests and of tools/mces_bench.py, and the hand table.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import graph_mirror as GM

W = GM.W
VALENCE = {1: 4, 2: 3, 3: 2, 4: 1}          # decoder types C, N, O, F (0 is H)


def kept_graph(mol, drop_h=True):
    """(types [m], weights [m, m] symmetric int, kept original indices [m]) of the atoms that take part."""
    n = len(mol["type"])
    t = np.asarray(mol["type"]).astype(np.int64)[:n]
    b = np.asarray(mol["bond"]).astype(np.int64)[:n, :n] & 255
    up = np.triu(b, 1)
    w = up + up.T
    keep = np.nonzero(t != 0)[0] if drop_h else np.arange(n)
    return t[keep], w[np.ix_(keep, keep)], keep


def total_weight(mol, drop_h=True):
    return int(kept_graph(mol, drop_h)[1].sum()) // 2


def _bonds(w):
    return [(int(i), int(j)) for i, j in np.argwhere(np.triu(w, 1) > 0)]


def score_of_map(a, b, image, drop_h=True):
    """score(pi) of a map over ORIGINAL indices (``image[i]`` = atom of ``b`` or -1), recomputed from the molecules; raises if the map is not
    injective, leaves its side, maps a dropped atom or changes a type - the check a test runs on what the kernel returned."""
    ta, wa, ka = kept_graph(a, drop_h)
    tb, wb, kb = kept_graph(b, drop_h)
    image = [int(x) for x in image]
    na = len(a["type"])
    assert all(x == -1 for x in image[na:]), "an atom beyond n is mapped"
    hit = [x for x in image[:na] if x != -1]
    assert len(set(hit)) == len(hit), "not injective"
    pos_a, pos_b = {int(o): c for c, o in enumerate(ka)}, {int(o): c for c, o in enumerate(kb)}
    for i in range(na):
        if image[i] != -1:
            assert i in pos_a and image[i] in pos_b, "a dropped or absent atom is mapped"
            assert ta[pos_a[i]] == tb[pos_b[image[i]]], "the map changes a type"
    total = 0
    for i, j in _bonds(wa):
        k, l = image[int(ka[i])], image[int(ka[j])]
        if k != -1 and l != -1:
            total += min(int(wa[i, j]), int(wb[pos_b[k], pos_b[l]]))
    return total


def mces_milp(a, b, drop_h=True):
    """dist by the integer program (exact: HiGHS proves optimality; the objective is an integer)."""
    from scipy.optimize import Bounds, LinearConstraint, milp
    from scipy.sparse import coo_matrix
    ta, wa, _ = kept_graph(a, drop_h)
    tb, wb, _ = kept_graph(b, drop_h)
    ea, eb = _bonds(wa), _bonds(wb)
    total = int(wa.sum()) // 2 + int(wb.sum()) // 2
    y = {}
    for i in range(len(ta)):
        for k in range(len(tb)):
            if ta[i] == tb[k]:
                y[i, k] = len(y)
    c, gain = {}, []
    for e, (i, j) in enumerate(ea):
        for f, (k, l) in enumerate(eb):
            if sorted((ta[i], ta[j])) == sorted((tb[k], tb[l])):
                c[e, f] = len(y) + len(c)
                gain.append(min(int(wa[i, j]), int(wb[k, l])))
    if not c:
        return total
    nv = len(y) + len(c)
    rows, cols, vals, ub = [], [], [], []

    def row(terms, bound):
        for col, v in terms:
            rows.append(len(ub)); cols.append(col); vals.append(v)
        ub.append(bound)
    for i in range(len(ta)):
        row([(v, 1.0) for (ii, _), v in y.items() if ii == i], 1.0)
    for k in range(len(tb)):
        row([(v, 1.0) for (_, kk), v in y.items() if kk == k], 1.0)
    for e in range(len(ea)):
        row([(v, 1.0) for (ee, _), v in c.items() if ee == e], 1.0)
    for f in range(len(eb)):
        row([(v, 1.0) for (_, ff), v in c.items() if ff == f], 1.0)
    for (e, f), v in c.items():
        (i, j), (k, l) = ea[e], eb[f]
        for end in (i, j):
            row([(v, 1.0)] + [(y[end, x], -1.0) for x in (k, l) if (end, x) in y], 0.0)
    A = coo_matrix((vals, (rows, cols)), shape=(len(ub), nv)).tocsr()
    obj = np.zeros(nv)
    obj[len(y):] = -np.asarray(gain, float)
    res = milp(obj, constraints=LinearConstraint(A, -np.inf, np.asarray(ub)), integrality=np.ones(nv), bounds=Bounds(0, 1))
    assert res.status == 0, res.message
    best = int(round(-res.fun))
    assert abs(-res.fun - best) < 1e-6
    return total - 2 * best


def mces_exhaustive(a, b, drop_h=True):
    """dist by enumerating every partial injective type-preserving map."""
    ta, wa, _ = kept_graph(a, drop_h)
    tb, wb, _ = kept_graph(b, drop_h)
    na, nb = len(ta), len(tb)
    ea = _bonds(wa)
    image, used = [-1] * na, [False] * nb
    best = 0

    def place(i):
        nonlocal best
        if i == na:
            s = sum(min(int(wa[p, q]), int(wb[image[p], image[q]])) for p, q in ea if image[p] >= 0 and image[q] >= 0)
            best = max(best, s)
            return
        place(i + 1)
        for k in range(nb):
            if not used[k] and ta[i] == tb[k]:
                image[i], used[k] = k, True
                place(i + 1)
                image[i], used[k] = -1, False
    place(0)
    return int(wa.sum()) // 2 + int(wb.sum()) // 2 - 2 * best


# ------------------------------------------------------------------------------------------------------------------ molecules

def random_molecule(rng, heavy, max_atoms=W):
    """A molecule-like graph of ``heavy`` atoms of C, N, O, F under their valences: a tree, 0-3 ring closures, 0-3 raised bond orders, then
    hydrogens on the free valences while the molecule has fewer than ``max_atoms`` atoms."""
    while True:
        types = [int(t) for t in rng.choice([1, 1, 1, 1, 2, 2, 3, 3, 4], size=heavy)]
        free = [VALENCE[t] for t in types]
        bond = np.zeros((heavy, heavy), np.int64)
        ok = True
        for v in range(1, heavy):
            open_ = [u for u in range(v) if free[u] > 0]
            if not open_:
                ok = False
                break
            u = open_[int(rng.integers(len(open_)))]
            bond[u, v] = bond[v, u] = 1
            free[u] -= 1
            free[v] -= 1
        if ok:
            break
    for _ in range(int(rng.integers(0, 4))):
        cand = [(i, j) for i in range(heavy) for j in range(i + 1, heavy) if bond[i, j] == 0 and free[i] > 0 and free[j] > 0]
        if not cand:
            break
        i, j = cand[int(rng.integers(len(cand)))]
        bond[i, j] = bond[j, i] = 1
        free[i] -= 1
        free[j] -= 1
    for _ in range(int(rng.integers(0, 4))):
        cand = [(i, j) for i in range(heavy) for j in range(i + 1, heavy) if 0 < bond[i, j] < 3 and free[i] > 0 and free[j] > 0]
        if not cand:
            break
        i, j = cand[int(rng.integers(len(cand)))]
        bond[i, j] += 1
        bond[j, i] += 1
        free[i] -= 1
        free[j] -= 1
    edges = []
    for i in range(heavy):
        for _ in range(free[i]):
            if len(types) < max_atoms:
                edges.append((i, len(types)))
                types.append(0)
    n = len(types)
    full = np.zeros((n, n), np.int64)
    full[:heavy, :heavy] = bond
    for i, h in edges:
        full[i, h] = full[h, i] = 1
    return dict(pos=np.zeros((n, 3)), type=np.asarray(types, np.int64), fc=np.zeros(n, np.int64), bond=full)


def treated(mol, kind, rng, heavy_range, max_atoms):
    """The generated side: 0 the molecule itself, 1 one heavy-atom bond moved, 2 one heavy-atom bond order changed, 3 one heavy type changed,
    4 an unrelated molecule; then the atoms are renamed.  (No valence repair: the hydrogens stay where they were.)"""
    m = dict(pos=mol["pos"], type=mol["type"].copy(), fc=mol["fc"].copy(), bond=mol["bond"].copy())
    heavy = np.nonzero(m["type"] != 0)[0]
    bonds = [(i, j) for i in heavy for j in heavy if i < j and m["bond"][i, j] > 0]
    if kind == 1 and bonds:
        gaps = [(i, j) for i in heavy for j in heavy if i < j and m["bond"][i, j] == 0]
        if gaps:
            (i, j), (k, l) = bonds[int(rng.integers(len(bonds)))], gaps[int(rng.integers(len(gaps)))]
            m["bond"][k, l] = m["bond"][l, k] = m["bond"][i, j]
            m["bond"][i, j] = m["bond"][j, i] = 0
    elif kind == 2 and bonds:
        i, j = bonds[int(rng.integers(len(bonds)))]
        m["bond"][i, j] = m["bond"][j, i] = m["bond"][i, j] % 3 + 1
    elif kind == 3:
        i = heavy[int(rng.integers(len(heavy)))]
        m["type"][i] = m["type"][i] % 4 + 1
    elif kind == 4:
        m = random_molecule(rng, int(rng.integers(heavy_range[0], heavy_range[1] + 1)), max_atoms)
    return GM.permuted(m, rng)


@functools.lru_cache(maxsize=8)
def seeded_pairs(count=600, seed=20261101, heavy=(1, 9), max_atoms=W):
    """(ground truths, generated molecules, kind [count]): ``random_molecule`` of ``heavy[0]..heavy[1]`` heavy atoms, the generated side
    ``treated`` with kind p % 5.  What a pair's distance is decides ``mces_milp``, not the recipe."""
    rng = np.random.default_rng(seed)
    ref, prb, kind = [], [], []
    for p in range(count):
        mol = random_molecule(rng, int(rng.integers(heavy[0], heavy[1] + 1)), max_atoms)
        ref.append(mol)
        kind.append(p % 5)
        prb.append(treated(mol, kind[-1], rng, heavy, max_atoms))
    return ref, prb, np.array(kind)


@functools.lru_cache(maxsize=8)
def seeded_distances(count=600, seed=20261101, heavy=(1, 9), max_atoms=W, drop_h=True):
    """``mces_milp`` of every seeded pair (generated molecule first, as the kernel takes them), computed once per process."""
    ref, prb, _ = seeded_pairs(count, seed, heavy, max_atoms)
    return np.array([mces_milp(a, b, drop_h) for a, b in zip(prb, ref)], np.int64)


# ------------------------------------------------------------------------------------------------------------------ the hand table

def _mol(types, edges, orders=None):
    return GM.molecule(types, edges, orders=orders)


def hand_table():
    """[(name, molecule, molecule, dist)] with hydrogens left out (heavy atoms only; the values hold with ``drop_h`` 0 and 1 alike)."""
    ring = GM._path(0, 1, 2, 3, 4, 5, 0)
    xylene = ring + [(0, 6), (1, 7)]                # the two methyls sit on ring atoms 0 and 1
    kek = lambda first: [2 if k % 2 == first else 1 for k in range(6)]
    return [
        ("ethane / ethene", _mol([1, 1], [(0, 1)]), _mol([1, 1], [(0, 1)], [2]), 1),
        ("propane / cyclopropane", _mol([1, 1, 1], [(0, 1), (1, 2)]), _mol([1, 1, 1], [(0, 1), (1, 2), (0, 2)]), 1),
        ("ethanol / dimethyl ether", _mol([1, 1, 3], [(0, 1), (1, 2)]), _mol([1, 3, 1], [(0, 1), (1, 2)]), 2),
        ("benzene Kekule / the shifted Kekule", _mol([1] * 6, ring, kek(0)), _mol([1] * 6, ring, kek(1)), 0),
        ("hexagon / two triangles", GM.carbons(6, ring), GM.carbons(6, GM._path(0, 1, 2, 0) + GM._path(3, 4, 5, 3)), 4),
        ("acetic acid / methyl formate", _mol([1, 1, 3, 3], [(0, 1), (1, 2), (1, 3)], [1, 2, 1]),
         _mol([1, 3, 1, 3], [(0, 1), (1, 2), (2, 3)], [1, 1, 2]), 2),
        ("ethane / methanol", _mol([1, 1], [(0, 1)]), _mol([1, 3], [(0, 1)]), 2),
        ("methane / water", _mol([1], []), _mol([3], []), 0),
        ("o-xylene, two Kekule drawings", _mol([1] * 8, xylene, kek(0) + [1, 1]), _mol([1] * 8, xylene, kek(1) + [1, 1]), 2),
    ]
