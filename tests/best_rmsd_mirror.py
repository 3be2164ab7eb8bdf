"""CPU yardstick of ``dsr_best_rmsd_records`` (include/diffspectra_rmsd.h) in plain numpy float64, independent of the colour refinement: a
backtracking enumeration of every label- and bond-preserving bijection, a Kabsch fit by ``numpy.linalg.svd`` per selected-atom map, and the
value as the EXPLICIT residual of the fitted rotation (not the trace formula the kernel uses).  In HEAVY mode the maps of the selected atoms
are enumerated first and the extension to the hydrogens is enumerated below each of them, so the fit runs once per heavy map.

A molecule is the dict of tests/structure_mirror.py (``pos`` = the fp32 values of the record as float64, ``type``, ``fc``, ``bond``).  Also here:
the hand molecules, the treatments and the seeded pair set that the CPU and GPU tests share."""
from __future__ import annotations

import functools

import numpy as np

from tests import stereo_mirror as K
from tests import structure_mirror as SM

W = SM.W
DIFFERENT, DECIDED, UNDECIDED, INVALID = range(4)
H, C, N, O, F = range(5)
BOUND_FACTOR = 256.0 * 2.0 ** -53          # |got^2 - want^2| <= BOUND_FACTOR * G / count: the rounding bound of the trace formula


def _bonds(mol):
    n = len(mol["type"])
    up = np.triu(np.asarray(mol["bond"]).astype(np.int64)[:n, :n] & 255, 1)
    return (up + up.T).tolist()


def selection(mol, atoms):
    """Indices of the selected atoms: type byte not 0 (``'heavy'``) or all of them (``'all'``)."""
    return [i for i in range(len(mol["type"])) if atoms == "all" or (int(mol["type"][i]) & 255) != 0]


def ordinals(mol, atoms):
    """HEAVY mode: the rank of every hydrogen leaf among its twins (type byte 0, exactly one bond, the same parent, bond byte and charge
    byte), 0 for every other atom.  ALL mode: zeros."""
    n, B = len(mol["type"]), _bonds(mol)
    if atoms == "all":
        return [0] * n
    key = []
    for i in range(n):
        nb = [j for j in range(n) if B[i][j] > 0]
        leaf = (int(mol["type"][i]) & 255) == 0 and len(nb) == 1
        key.append((nb[0], B[i][nb[0]], int(mol["fc"][i]) & 255) if leaf else ("self", i))
    return [sum(1 for j in range(i) if key[j] == key[i]) for i in range(n)]


def centred(mol, atoms):
    """[n, 3] float64: the selected positions minus the centroid of the selection, zero rows for the other atoms."""
    pos = np.asarray(mol["pos"], np.float64)
    out = np.zeros_like(pos)
    sel = selection(mol, atoms)
    if sel:
        out[sel] = pos[sel] - pos[sel].mean(axis=0)
    return out


def fit(xa, xb):
    """(proper, improper) sums of squared residuals of the rows ``xa`` fitted onto ``xb`` (both centred) by the best rotation / the best
    rotation after a reflection: Kabsch by numpy's SVD, the residual taken explicitly."""
    if len(xa) == 0:
        return 0.0, 0.0
    U, _, Vt = np.linalg.svd(xa.T @ xb)
    sign = 1.0 if np.linalg.det(U) * np.linalg.det(Vt) >= 0 else -1.0
    out = []
    for d in (sign, -sign):
        Q = U @ np.diag([1.0, 1.0, d]) @ Vt
        out.append(float(((xa @ Q - xb) ** 2).sum()))
    return out[0], out[1]


def values_of_map(a, b, image, atoms):
    """(proper, improper) RMSD of one map (``image[i]`` = atom of ``b`` for atom ``i`` of ``a``): numpy Kabsch, explicit residuals.  NaN for an
    empty selection."""
    sel = selection(a, atoms)
    if not sel:
        return float("nan"), float("nan")
    xa, xb = centred(a, atoms)[sel], centred(b, atoms)[[int(image[i]) for i in sel]]
    p, q = fit(xa, xb)
    return float(np.sqrt(p / len(sel))), float(np.sqrt(q / len(sel)))


def scale_of(a, b, atoms):
    """(G, count) of a pair: G = sum |a_i|^2 + sum |b_i|^2 over the centred selections, count = selected atoms of ``a``."""
    return float((centred(a, atoms) ** 2).sum() + (centred(b, atoms) ** 2).sum()), len(selection(a, atoms))


def bound_of(a, b, atoms):
    """The bound on |got^2 - want^2| of this pair (inf for an empty selection, where both are NaN)."""
    G, count = scale_of(a, b, atoms)
    return BOUND_FACTOR * G / count if count else float("inf")


def _enumerate(a, b, atoms):
    """Yields (selected image tuple, number of ordinal-respecting extensions to all atoms, one such extension) for every map of the selected
    atoms of ``a`` into ``b`` that extends to an isomorphism: plain backtracking, the selected atoms placed first."""
    n = len(a["type"])
    A, B = _bonds(a), _bonds(b)
    oa, ob = ordinals(a, atoms), ordinals(b, atoms)
    la = [(int(a["type"][i]) & 255, int(a["fc"][i]) & 255, oa[i], sum(1 for x in A[i] if x)) for i in range(n)]
    lb = [(int(b["type"][i]) & 255, int(b["fc"][i]) & 255, ob[i], sum(1 for x in B[i] if x)) for i in range(n)]
    if sorted(la) != sorted(lb):
        return
    sel = selection(a, atoms)
    chosen = set(sel)

    def connected(first):                      # breadth first inside `first`, every new piece from its lowest atom
        order, seen = [], set()
        for s in first:
            if s in seen:
                continue
            seen.add(s)
            queue = [s]
            while queue:
                v = queue.pop(0)
                order.append(v)
                for u in first:
                    if A[v][u] and u not in seen:
                        seen.add(u)
                        queue.append(u)
        return order
    rest = [i for i in range(n) if i not in chosen]
    order = connected(sel) + sorted(rest, key=lambda i: (min([j for j in range(n) if A[i][j]] + [n]), i))
    image, used = [-1] * n, [False] * n

    def place(k, stop):
        if k == stop:
            yield None
            return
        v = order[k]
        for w in range(n):
            if used[w] or la[v] != lb[w]:
                continue
            if any(A[v][order[q]] != B[w][image[order[q]]] for q in range(k)):
                continue
            image[v], used[w] = w, True
            yield from place(k + 1, stop)
            image[v], used[w] = -1, False

    for _ in place(0, len(sel)):
        count, one = 0, None
        for _ in place(len(sel), n):
            count += 1
            if one is None:
                one = list(image)
        if count:
            yield tuple(image[i] for i in sel), count, one


def compare(a, b, atoms="heavy"):
    """What the header defines for one pair whose search ends: ``verdict`` (0 / 1), ``count``, ``found`` (ordinal-respecting isomorphisms),
    ``best`` / ``runner_up`` (per kind, proper then improper: the smallest and the second smallest value over the distinct maps of the selected
    atoms, inf without a second), ``optimal`` (per kind: the set of selected-image tuples within 1e-9 of the best), ``maps`` (the number of
    distinct selected maps), ``selected`` (the selected atoms of ``a``), ``G``."""
    G, count = scale_of(a, b, atoms) if len(a["type"]) == len(b["type"]) else (float("nan"), len(selection(a, atoms)))
    out = dict(verdict=DIFFERENT, count=count, found=0, best=[float("nan")] * 2, runner_up=[float("inf")] * 2, optimal=[set(), set()], maps=0,
               selected=selection(a, atoms), G=G)
    if len(a["type"]) != len(b["type"]):
        return out
    xa, xb = centred(a, atoms), centred(b, atoms)
    sel = out["selected"]
    scored = []
    for images, ways, _ in _enumerate(a, b, atoms):
        out["found"] += ways
        p, q = fit(xa[sel], xb[list(images)])
        scored.append((images, p, q))
    if not scored:
        return out
    out["verdict"], out["maps"] = DECIDED, len(scored)
    for kind in (0, 1):
        if not count:
            out["optimal"][kind] = {s[0] for s in scored}
            continue
        vals = sorted(float(np.sqrt(s[1 + kind] / count)) for s in scored)
        out["best"][kind] = vals[0]
        out["runner_up"][kind] = vals[1] if len(vals) > 1 else float("inf")
        out["optimal"][kind] = {s[0] for s in scored if np.sqrt(s[1 + kind] / count) <= vals[0] + 1e-9}
    return out


def is_isomorphism(a, b, image, atoms):
    """A map the kernel returned: a bijection that preserves type, charge byte, every bond byte and (HEAVY mode) the hydrogen ordinals."""
    n = len(a["type"])
    image = [int(x) for x in image[:n]]
    if len(b["type"]) != n or sorted(image) != list(range(n)) or any(int(x) != -1 for x in image[n:]):
        return False
    A, B = _bonds(a), _bonds(b)
    oa, ob = ordinals(a, atoms), ordinals(b, atoms)
    same = all((int(a["type"][i]) & 255, int(a["fc"][i]) & 255, oa[i]) == (int(b["type"][image[i]]) & 255, int(b["fc"][image[i]]) & 255, ob[image[i]])
               for i in range(n))
    return same and all(A[i][j] == B[image[i]][image[j]] for i in range(n) for j in range(n))


# ------------------------------------------------------------------------------------------------------------------ treatments

def moved(mol, rng, noise=0.0):
    """A random proper rotation, a shift, a renumbering, then Gaussian noise of ``noise`` A per coordinate; fp32 values, as a record holds."""
    out = K.renumbered(mol, rng)
    if noise:
        out["pos"] = K._f32(out["pos"] + rng.normal(size=out["pos"].shape) * noise)
    return out


def reflected(mol):
    return K.reflected(mol)                    # x -> -x: exact in fp32


# ------------------------------------------------------------------------------------------------------------------ hand molecules

def _mol(types, pos, edges, orders=None):
    b = K.Builder()
    for t, p in zip(types, pos):
        b.atom(t, p)
    for k, (i, j) in enumerate(edges):
        b.bond(i, j, 1 if orders is None else orders[k])
    return b.done()


def diatomic(d, types=(C, O)):
    return _mol(types, [(0, 0, 0), (d, 0, 0)], [(0, 1)])


def triangle(s):
    """Cyclopropane skeleton without hydrogens: an equilateral triangle of side ``s``."""
    r = s / np.sqrt(3.0)
    return _mol([C] * 3, [(r * np.cos(t), r * np.sin(t), 0.0) for t in (0.0, 2 * np.pi / 3, 4 * np.pi / 3)], [(0, 1), (1, 2), (0, 2)])


def four_heavy(r=1.4):
    """A carbon with four different heavy substituents (N, O, F, C) on an ideal tetrahedron of radius ``r``."""
    return _mol([C, N, O, F, C], [(0, 0, 0)] + [K.T[k] * r for k in range(4)], [(0, 1), (0, 2), (0, 3), (0, 4)])


def cf2h2(r1=1.30, r2=1.40):
    """CF2H2 with C-F lengths ``r1`` (atom 1) and ``r2`` (atom 2)."""
    return _mol([C, F, F, H, H], [(0, 0, 0), K.T[0] * r1, K.T[1] * r2, K.T[2] * 1.1, K.T[3] * 1.1], [(0, 1), (0, 2), (0, 3), (0, 4)])


def swapped(mol, i, j):
    """Atoms ``i`` and ``j`` exchange their indices (positions, labels and bonds go with them)."""
    perm = np.arange(len(mol["type"]))
    perm[[i, j]] = perm[[j, i]]
    return dict(pos=mol["pos"][perm].copy(), type=mol["type"][perm].copy(), fc=mol["fc"][perm].copy(), bond=np.asarray(mol["bond"])[np.ix_(perm, perm)].copy())


def water():
    return _mol([O, H, H], [(0, 0, 0), (0.76, 0.59, 0), (-0.76, 0.59, 0)], [(0, 1), (0, 2)])


def h2():
    return _mol([H, H], [(0, 0, 0), (0.74, 0, 0)], [(0, 1)])


def ethane():
    b = K.Builder()
    c0 = b.methyl((0, 0, 0), None, 1, 0)
    b.methyl(-K.T[0] * 1.5, c0, -1, 0)
    return b.done()


def benzene():
    """Kekule benzene: alternating bond bytes 2 and 1, so its graph has the 6 automorphisms that keep the alternation."""
    b = K.Builder()
    ring = [(np.cos(k * np.pi / 3), np.sin(k * np.pi / 3), 0.0) for k in range(6)]
    c = [b.atom(C, np.asarray(p) * 1.39) for p in ring]
    for k in range(6):
        b.bond(c[k], c[(k + 1) % 6], 2 if k % 2 == 0 else 1)
    for k in range(6):
        b.atom(H, np.asarray(ring[k]) * 2.48, c[k])
    return b.done()


def cyclohexane():
    """The chair: ring carbons alternately above and below the mean plane, an axial and an equatorial hydrogen on each."""
    b = K.Builder()
    ring = [np.array((1.45 * np.cos(k * np.pi / 3), 1.45 * np.sin(k * np.pi / 3), 0.25 * (-1) ** k)) for k in range(6)]
    c = [b.atom(C, p) for p in ring]
    for k in range(6):
        b.bond(c[k], c[(k + 1) % 6])
    for k in range(6):
        b.atom(H, ring[k] + (0, 0, 1.1 * (-1) ** k), c[k])
        b.atom(H, ring[k] * (1 + 1.05 / 1.47) - (0, 0, 0.35 * (-1) ** k), c[k])
    return b.done()


def tetramethylbutane():
    """2,2,3,3-tetramethylbutane, (CH3)3C-C(CH3)3: 26 atoms, 72 heavy automorphisms."""
    b = K.Builder()
    c0 = b.atom(C, (0, 0, 0))
    c1 = b.atom(C, K.T[0] * 1.55, c0)
    for k in (1, 2, 3):
        b.methyl(K.T[k] * 1.5, c0, 1, k)
    for k in (1, 2, 3):
        b.methyl(K.T[0] * 1.55 - K.T[k] * 1.5, c1, -1, k)
    return b.done()


def skeletons():
    """(name, molecule, heavy ``found`` or None) of the symmetric skeletons of the hand table."""
    return [("cubane", K.cubane(), 48), ("neopentane", K.neopentane(), 24), ("benzene", benzene(), 6), ("cyclohexane", cyclohexane(), 12),
            ("tetramethylbutane", tetramethylbutane(), 72)]


def hand_pairs():
    """(name, generated, ground truth, atoms) of the hand table that both test files run.  Closed forms and counts are asserted in
    tests/test_best_rmsd_cpu.py."""
    rng = np.random.default_rng(20261101)
    chiral = four_heavy()
    wat = water()
    big = tetramethylbutane()
    changed = dict(big, bond=np.asarray(big["bond"]).copy())
    changed["bond"][0, 1] = changed["bond"][1, 0] = 2
    rows = [("two atoms", diatomic(1.1), diatomic(1.5), "heavy"), ("two atoms, all", diatomic(1.1), diatomic(1.5), "all"),
            ("triangles", triangle(1.5), triangle(1.8), "heavy"),
            ("four heavy substituents / mirror image", moved(reflected(chiral), rng), chiral, "heavy"),
            ("CF2H2, F swapped", swapped(cf2h2(), 1, 2), cf2h2(), "heavy"), ("CF2H2, F swapped, all", swapped(cf2h2(), 1, 2), cf2h2(), "all"),
            ("water, H renumbered, all", swapped(wat, 1, 2), wat, "all"), ("H2, heavy", h2(), h2(), "heavy"), ("H2, all", h2(), h2(), "all"),
            ("one heavy atom", _mol([N], [(1, 2, 3)], []), _mol([N], [(0, 0, 0)], []), "heavy"),
            ("one atom against two", _mol([N], [(1, 2, 3)], []), diatomic(1.1), "heavy"),
            ("a changed bond byte", changed, big, "heavy"), ("ethane, all", moved(ethane(), rng, 0.05), ethane(), "all")]
    for name, mol, _ in skeletons():
        rows.append((name, moved(mol, rng, 0.1), mol, "heavy"))
    rows.append(("benzene, all", moved(benzene(), rng, 0.1), benzene(), "all"))
    return rows


# ------------------------------------------------------------------------------------------------------------------ the seeded set

SEED = 20261102
N_PAIRS, N_FULL = 600, 48                   # pairs; of them with n = 29 (lane 28, LDS row 28)
HEAVY_LIMIT = 96                            # a symmetric skeleton's product of the heavy leaf-twin factorials is at most this
ALL_LIMIT = 48                              # the ALL mode runs where the product of the leaf-twin factorials is at most this


def _tree(rng, n):
    pos, types, fc, bond = SM.random_tree_molecule(rng, n)
    return dict(pos=K._f32(pos), type=types, fc=fc, bond=bond)


def _spoiled(mol, rng):
    """One type, one charge or one bond byte changed."""
    out = dict(pos=mol["pos"].copy(), type=mol["type"].copy(), fc=mol["fc"].copy(), bond=np.asarray(mol["bond"]).copy())
    n, what = len(mol["type"]), int(rng.integers(3))
    i = int(rng.integers(n))
    if what == 0:
        out["type"][i] = (out["type"][i] + 1 + int(rng.integers(4))) % 5
    elif what == 1:
        out["fc"][i] = out["fc"][i] + 1 if out["fc"][i] <= 0 else -1
    else:
        pairs = np.argwhere(np.triu(out["bond"]) > 0)
        i, j = pairs[int(rng.integers(len(pairs)))]
        out["bond"][i, j] = out["bond"][j, i] = out["bond"][i, j] % 3 + 1
    return out


def _plain(mol, rng):
    """The tree as a symmetric skeleton: no charges, single bonds, carbon inside, and H, H, C or F on every leaf."""
    n, bond = len(mol["type"]), (np.asarray(mol["bond"]) > 0).astype(np.int64)
    leaf = bond.sum(1) == 1
    types = np.where(leaf, rng.choice([H, H, C, F], size=n), C).astype(np.int64)
    return dict(pos=mol["pos"], type=types, fc=np.zeros(n, np.int64), bond=bond)


def _leaf_twin_product(mol, heavy_only=False):
    from math import factorial
    n, B = len(mol["type"]), _bonds(mol)
    groups = {}
    for i in range(n):
        nb = [j for j in range(n) if B[i][j]]
        if len(nb) == 1 and not (heavy_only and int(mol["type"][i]) == 0):
            k = (nb[0], B[i][nb[0]], int(mol["type"][i]), int(mol["fc"][i]))
            groups[k] = groups.get(k, 0) + 1
    return int(np.prod([factorial(v) for v in groups.values()])) if groups else 1


@functools.lru_cache(maxsize=1)
def seeded_pairs():
    """(generated, ground truth, kinds) of ``N_PAIRS`` seeded pairs: random trees of 3-29 atoms (``N_FULL`` of them with 29; every third one a
    symmetric skeleton: carbon inside, H / C / F leaves, single bonds, no charges - heavy leaf twins, equal branches), the generated side moved rigidly, renumbered and noised by 0.02 / 0.1 / 0.3 / 0.6 A; every fourth pair spoiled (a changed type, charge or bond byte:
    verdict 0 unless the change is an automorphic accident), every tenth reflected.  ``kinds[p]`` is 'copy', 'spoiled' or 'reflected'."""
    rng = np.random.default_rng(SEED)
    prb, ref, kinds = [], [], []
    for p in range(N_PAIRS):
        n = W if p % (N_PAIRS // N_FULL) == 0 else int(rng.integers(3, W + 1))
        truth = _tree(rng, n)
        while p % 3 == 0:                       # every third pair a symmetric skeleton, redrawn until its heavy leaf twins stay few
            truth = _plain(truth, rng)
            if _leaf_twin_product(truth, heavy_only=True) <= HEAVY_LIMIT:
                break
            truth = _tree(rng, n)
        made, kind = truth, "copy"
        if p % 4 == 1:
            made, kind = _spoiled(truth, rng), "spoiled"
        elif p % 10 == 2:
            made, kind = reflected(truth), "reflected"
        prb.append(moved(made, rng, (0.02, 0.1, 0.3, 0.6)[(p // 4) % 4]))
        ref.append(truth)
        kinds.append(kind)
    return prb, ref, kinds


@functools.lru_cache(maxsize=2)
def seeded_results(atoms):
    """``compare`` of every seeded pair that runs in this mode (``None`` for a pair left out of the ALL mode), computed once."""
    prb, ref, _ = seeded_pairs()
    return [compare(a, b, atoms) if atoms == "heavy" or _leaf_twin_product(b) <= ALL_LIMIT else None for a, b in zip(prb, ref)]
