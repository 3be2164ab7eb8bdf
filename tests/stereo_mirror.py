"""CPU yardstick of ``dsc_stereo_identity_records`` and ``dsc_stereo_sites`` (include/diffspectra_stereo.h), in plain Python and numpy float64.

Written from the header, not from the kernel: every ordinal-respecting isomorphism is enumerated by textbook backtracking (atoms of the
first molecule in a connected order, each tried on every unused atom of the second with the same type, charge, ordinal and degree whose
bonds to the atoms mapped so far agree) - no colour refinement, no individualisation - and every isomorphism is tested against the sites by
GEOMETRY: the volume of the ground truth's centre is recomputed with its neighbours in the order of the images, the cis bit of the images is
read off their own cosine.  The kernel does both in integers (parity of the images, flips from the lowest substituent), so an agreement of the
two is evidence for both.  A molecule is the dict of ``structure_mirror.mol_from_record`` (``pos [n,3] f64 holding fp32 values, type [n], fc
[n], bond [n,n]``).

Also here: the hand table (molecules from simple constructions - only signs matter, so they are not realistic), the treatments (rigid motion
plus renumbering, reflection, swapping two neighbours of a centre) and the seeded pair set that the CPU and the GPU tests share.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import graph_mirror as GM
from tests import structure_mirror as SM

W = SM.W
DIFFERENT, IDENTICAL, UNDECIDED, INVALID, MIRROR, STEREOISOMER, UNASSIGNED = range(7)
MIN_VOLUME = MIN_PLANARITY = 0.5
H, C, N, O, F = range(5)


# ------------------------------------------------------------------------------------------------------------------ perception

def _bonds(mol):
    """Bond bytes as a symmetric integer matrix: the upper triangle of the record's matrix decides, the diagonal is no pair."""
    n = len(mol["type"])
    up = np.triu(np.asarray(mol["bond"]).astype(np.int64)[:n, :n] & 255, 1)
    return up + up.T


def _labels(mol):
    n = len(mol["type"])
    return [(int(mol["type"][i]) & 255, int(mol["fc"][i]) & 255) for i in range(n)]


def twins_of(mol):
    """(are_twins(i, j), ordinal [n], twin [n]) by the header's two rules."""
    n, B, lab = len(mol["type"]), _bonds(mol), _labels(mol)
    nbrs = [[j for j in range(n) if B[i, j] > 0] for i in range(n)]

    def are_twins(i, j):
        if i == j or lab[i] != lab[j] or len(nbrs[i]) != len(nbrs[j]):
            return False
        if len(nbrs[i]) == 0:
            return True
        return len(nbrs[i]) == 1 and nbrs[i][0] == nbrs[j][0] and B[i, nbrs[i][0]] == B[j, nbrs[j][0]]

    twin = [any(are_twins(i, j) for j in range(n)) for i in range(n)]
    ordinal = [sum(1 for j in range(i) if are_twins(i, j)) for i in range(n)]
    return are_twins, ordinal, twin


def volume(pos, a, order):
    """V of centre ``a`` with its four neighbours in ``order``: (u1 - u4) . ((u2 - u4) x (u3 - u4)) over the unit vectors; may be NaN."""
    with np.errstate(all="ignore"):
        u = [(pos[j] - pos[a]) / np.sqrt(((pos[j] - pos[a]) ** 2).sum()) for j in order]
        return float(np.dot(u[0] - u[3], np.cross(u[1] - u[3], u[2] - u[3])))


def cosine(pos, a, b, s, t):
    """(c, usable) of substituent s of a and t of b around the bond a=b; usable = finite coordinates and two non-zero projections."""
    with np.errstate(all="ignore"):
        e = pos[b] - pos[a]
        v, w = pos[s] - pos[a], pos[t] - pos[b]
        p, q = v - e * (np.dot(v, e) / np.dot(e, e)), w - e * (np.dot(w, e) / np.dot(e, e))
        lp, lq = np.sqrt(np.dot(p, p)), np.sqrt(np.dot(q, q))
        c = float(np.dot(p, q) / (lp * lq))
    usable = bool(np.isfinite(pos[[a, b, s, t]]).all() and lp > 0 and lq > 0)
    return c, usable


def perceive(mol, min_volume=MIN_VOLUME, min_planarity=MIN_PLANARITY):
    """Twins, ordinals and sites of one molecule: dict(ordinal, twin, tetra = [dict(atom, nbrs, V, assigned, positive)], ez = [dict(a, b, subs_a,
    subs_b, assigned, cis)] with a < b, margin = the smallest distance of a |V| or |c| from its threshold)."""
    n, B = len(mol["type"]), _bonds(mol)
    pos = np.asarray(mol["pos"], np.float64)
    are_twins, ordinal, twin = twins_of(mol)
    nbrs = [[j for j in range(n) if B[i, j] > 0] for i in range(n)]
    no_twins = lambda atoms: not any(are_twins(i, j) for i in atoms for j in atoms)
    margin, tetra, ez = np.inf, [], []
    for a in range(n):
        if len(nbrs[a]) == 4 and no_twins(nbrs[a]):
            V = volume(pos, a, nbrs[a])
            fin = bool(np.isfinite(pos[[a] + nbrs[a]]).all())
            if np.isfinite(V):
                margin = min(margin, abs(abs(V) - min_volume))
            assigned = fin and abs(V) >= min_volume
            tetra.append(dict(atom=a, nbrs=nbrs[a], V=V, assigned=bool(assigned), positive=bool(assigned and V > 0)))

    def end(a, b):
        subs = [j for j in nbrs[a] if j != b]
        return subs if len(subs) in (1, 2) and all(B[a, j] < 2 for j in subs) and no_twins(subs) else None

    for a in range(n):
        for b in range(a + 1, n):
            if B[a, b] != 2:
                continue
            sa, sb = end(a, b), end(b, a)
            if sa is None or sb is None:
                continue
            ok, cis = True, {}
            for s in sa:
                for t in sb:
                    c, usable = cosine(pos, a, b, s, t)
                    if np.isfinite(c):
                        margin = min(margin, abs(abs(c) - min_planarity))
                    ok = ok and usable and abs(c) >= min_planarity
                    cis[s, t] = c > 0
            if len(sa) == 2:
                ok = ok and all(cis[sa[0], t] != cis[sa[1], t] for t in sb)
            if len(sb) == 2:
                ok = ok and all(cis[s, sb[0]] != cis[s, sb[1]] for s in sa)
            ez.append(dict(a=a, b=b, subs_a=sa, subs_b=sb, assigned=bool(ok), cis=bool(ok and cis[sa[0], sb[0]])))
    return dict(ordinal=ordinal, twin=twin, tetra=tetra, ez=ez, margin=float(margin))


def site_masks(mol, min_volume=MIN_VOLUME, min_planarity=MIN_PLANARITY):
    """What ``dsc_stereo_sites`` writes for one record: (masks [7] in the DSC_MASK_* order, volume [29], status)."""
    n, B = len(mol["type"]), _bonds(mol)
    vol = np.full(W, np.nan)
    if n == 0 or any(int(t) > 4 for t in mol["type"]) or (B > 3).any():
        return [0] * 7, vol, 3
    P = perceive(mol, min_volume, min_planarity)
    bits = lambda atoms: sum(1 << a for a in atoms)
    for s in P["tetra"]:
        vol[s["atom"]] = s["V"]
    ends = lambda key: [x for s in P["ez"] if key is None or s[key] for x in (s["a"], s["b"])]
    masks = [bits(s["atom"] for s in P["tetra"]), bits(s["atom"] for s in P["tetra"] if s["assigned"]), bits(s["atom"] for s in P["tetra"] if s["positive"]),
             bits(ends(None)), bits(ends("assigned")), bits(ends("cis")), bits(i for i in range(n) if P["twin"][i])]
    return masks, vol, 0


# ------------------------------------------------------------------------------------------------------------------ isomorphisms

def isomorphisms(a, b, ord_a, ord_b):
    """Every bijection of the atoms of ``a`` onto those of ``b`` that preserves type, charge byte, ordinal and the bond byte of every pair, as a
    list ``image`` with ``image[i]`` the atom of ``b`` that atom ``i`` of ``a`` goes to.  A generator: plain backtracking."""
    n = len(a["type"])
    if n != len(b["type"]):
        return
    A, B = _bonds(a), _bonds(b)
    la = [lab + (ord_a[i], int((A[i] > 0).sum())) for i, lab in enumerate(_labels(a))]
    lb = [lab + (ord_b[i], int((B[i] > 0).sum())) for i, lab in enumerate(_labels(b))]
    if sorted(la) != sorted(lb):
        return
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
                if A[v, u] and not seen[u]:
                    seen[u] = True
                    queue.append(u)
    image, used = [-1] * n, [False] * n

    def place(k):
        if k == n:
            yield list(image)
            return
        v = order[k]
        for w in range(n):
            if used[w] or la[v] != lb[w] or any(A[v, order[q]] != B[w, image[order[q]]] for q in range(k)):
                continue
            image[v], used[w] = w, True
            yield from place(k + 1)
            image[v], used[w] = -1, False

    yield from place(0)


def kind_of(b, pa, pb, image):
    """What the isomorphism ``image`` does to the sites (``pa`` / ``pb``: ``perceive`` of both molecules, all sites assigned): 'same', 'mirror' or
    'other' - from the geometry of ``b`` under the images, as the header defines it."""
    pos = np.asarray(b["pos"], np.float64)
    sign_b = {s["atom"]: s for s in pb["tetra"]}
    kept, turned = 0, 0
    for s in pa["tetra"]:
        target = image[s["atom"]]
        assert target in sign_b, "an isomorphism maps sites onto sites"
        positive = volume(pos, target, [image[j] for j in s["nbrs"]]) > 0
        kept += positive == s["positive"]
        turned += positive != s["positive"]
    ez_kept = True
    for s in pa["ez"]:
        c, _ = cosine(pos, image[s["a"]], image[s["b"]], image[s["subs_a"][0]], image[s["subs_b"][0]])
        ez_kept = ez_kept and (c > 0) == s["cis"]
    if turned == 0 and ez_kept:
        return "same"
    if pa["tetra"] and kept == 0 and ez_kept:
        return "mirror"
    return "other"


def compare(a, b, min_volume=MIN_VOLUME, min_planarity=MIN_PLANARITY):
    """One pair, ``a`` the generated molecule and ``b`` the ground truth, the search run to its end (``exhaustive = 1`` without a budget):
    dict(verdict, found [3], sites [4], margin, maps = {'iso': [...], 'same': [...], 'mirror': [...]})."""
    pa, pb = perceive(a, min_volume, min_planarity), perceive(b, min_volume, min_planarity)
    open_of = lambda p: sum(not s["assigned"] for s in p["tetra"]) + sum(not s["assigned"] for s in p["ez"])
    sites = [len(pa["tetra"]), len(pa["ez"]), open_of(pa), open_of(pb)]
    assigned = sites[2] + sites[3] == 0
    maps = dict(iso=[], same=[], mirror=[])
    for image in isomorphisms(a, b, pa["ordinal"], pb["ordinal"]):
        maps["iso"].append(image)
        if assigned:
            kind = kind_of(b, pa, pb, image)
            if kind != "other":
                maps[kind].append(image)
    if not maps["iso"]:
        verdict = DIFFERENT
    elif not assigned:
        verdict = UNASSIGNED
    else:
        verdict = IDENTICAL if maps["same"] else MIRROR if maps["mirror"] else STEREOISOMER
    return dict(verdict=verdict, found=[len(maps["iso"]), len(maps["same"]), len(maps["mirror"])], sites=sites,
                margin=min(pa["margin"], pb["margin"]), maps=maps)


def map_claim(a, b, image, verdict, min_volume=MIN_VOLUME, min_planarity=MIN_PLANARITY):
    """Does the map a kernel returned with ``verdict`` have the property the verdict claims?  An isomorphism that respects the ordinals for 1,
    4, 5 and 6 - a same one for 1, a mirror one for 4 -, all -1 for every other verdict."""
    n = len(a["type"])
    image = [int(x) for x in image]
    if verdict not in (IDENTICAL, MIRROR, STEREOISOMER, UNASSIGNED):
        return all(x == -1 for x in image)
    if any(x != -1 for x in image[n:]) or not GM.is_isomorphism(a, b, image[:n]):
        return False
    pa, pb = perceive(a, min_volume, min_planarity), perceive(b, min_volume, min_planarity)
    if any(pa["ordinal"][i] != pb["ordinal"][image[i]] for i in range(n)):
        return False
    if verdict in (IDENTICAL, MIRROR):
        return kind_of(b, pa, pb, image[:n]) == ("same" if verdict == IDENTICAL else "mirror")
    return True


# ------------------------------------------------------------------------------------------------------------------ treatments

def _f32(pos):
    return np.asarray(pos, np.float32).astype(np.float64)         # what a record holds


def renumbered(mol, rng):
    """The same molecule after a random proper rotation, a shift and a renumbering of its atoms: new atom i is old atom perm[i]."""
    n = len(mol["type"])
    perm = rng.permutation(n)
    pos = np.asarray(mol["pos"], np.float64) @ SM._rotation(rng) + rng.uniform(-2, 2, size=(1, 3))
    return dict(pos=_f32(pos[perm]), type=mol["type"][perm].copy(), fc=mol["fc"][perm].copy(), bond=np.asarray(mol["bond"])[np.ix_(perm, perm)].copy())


def reflected(mol):
    """The mirror image: x -> -x."""
    pos = np.asarray(mol["pos"], np.float64).copy()
    pos[:, 0] = -pos[:, 0]
    return dict(pos=pos, type=mol["type"].copy(), fc=mol["fc"].copy(), bond=np.asarray(mol["bond"]).copy())


def neighbours_swapped(mol, i, j):
    """The positions of atoms i and j exchanged (two neighbours of one site): the graph stays, that site inverts."""
    pos = np.asarray(mol["pos"], np.float64).copy()
    pos[[i, j]] = pos[[j, i]]
    return dict(pos=pos, type=mol["type"].copy(), fc=mol["fc"].copy(), bond=np.asarray(mol["bond"]).copy())


# ------------------------------------------------------------------------------------------------------------------ the hand table

T = np.array([(1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)], float) / np.sqrt(3.0)      # the four directions of a tetrahedron


class Builder:
    def __init__(self):
        self.type, self.pos, self.edges, self.orders = [], [], [], []

    def atom(self, element, pos, bonded_to=None, order=1):
        self.type.append(element)
        self.pos.append(np.asarray(pos, float))
        if bonded_to is not None:
            self.edges.append((bonded_to, len(self.type) - 1))
            self.orders.append(order)
        return len(self.type) - 1

    def bond(self, i, j, order=1):
        self.edges.append((i, j))
        self.orders.append(order)

    def methyl(self, at, bonded_to, sign, k):
        """CH3 at ``at``; its bond back points along -sign T[k], so its hydrogens sit along -sign T[j], j != k."""
        c = self.atom(C, at, bonded_to)
        for j in range(4):
            if j != k:
                self.atom(H, np.asarray(at) - sign * T[j] * 1.1, c)
        return c

    def done(self):
        mol = GM.molecule(self.type, self.edges, orders=self.orders)
        mol["pos"] = _f32(np.array(self.pos).reshape(-1, 3))
        return mol


def fluoroethanol(flat=False, double_co=False):
    """CH3-CH(F)(OH): one centre (atom 0).  ``flat``: its neighbours nearly in a plane; ``double_co``: the C-O bond of order 2 (another graph)."""
    m = Builder()
    c = m.atom(C, (0, 0, 0))
    spots = [(1.5, 0, 0), (0, 1.4, 0), (-1.4, 0, 0), (0, -1.1, 0.05)] if flat else [T[0] * 1.5, T[1] * 1.4, T[2] * 1.4, T[3] * 1.1]
    m.methyl(spots[0], c, 1, 0)
    m.atom(F, spots[1], c)
    o = m.atom(O, spots[2], c, 2 if double_co else 1)
    m.atom(H, spots[3], c)
    m.atom(H, np.asarray(spots[2]) + (-0.5, -0.8, 0.3), o)
    return m.done()


def difluorobutane(meso):
    """CH3-CHF-CHF-CH3 around the bond C0-C1 along T[0].  C0 carries (CH3, F, H) on T[1..3]; C1 carries them on -T[1..3] in the same order
    (an inversion centre: meso) or with CH3 and F exchanged (chiral)."""
    m = Builder()
    c0 = m.atom(C, (0, 0, 0))
    c1 = m.atom(C, T[0] * 1.5, c0)
    m.methyl(T[1] * 1.5, c0, 1, 1)
    m.atom(F, T[2] * 1.4, c0)
    m.atom(H, T[3] * 1.1, c0)
    at = lambda k, r: T[0] * 1.5 - T[k] * r
    k_me, k_f = (1, 2) if meso else (2, 1)
    m.methyl(at(k_me, 1.5), c1, -1, k_me)
    m.atom(F, at(k_f, 1.4), c1)
    m.atom(H, at(3, 1.1), c1)
    return m.done()


def difluorocyclobutane(cis):
    """A flat four-ring; C0 and C2 carry F and H above and below it, C1 and C3 two hydrogens (twins)."""
    m = Builder()
    ring = [(1, 0, 0), (0, 1, 0), (-1, 0, 0), (0, -1, 0)]
    c = [m.atom(C, p) for p in ring]
    for i in range(4):
        m.bond(c[i], c[(i + 1) % 4])
    up = lambda i, z: np.asarray(ring[i]) * 1.5 + (0, 0, z)
    m.atom(F, up(0, 0.9), c[0])
    m.atom(H, up(0, -0.9), c[0])
    m.atom(F, up(2, 0.9 if cis else -0.9), c[2])
    m.atom(H, up(2, -0.9 if cis else 0.9), c[2])
    for i in (1, 3):
        m.atom(H, up(i, 0.9), c[i])
        m.atom(H, up(i, -0.9), c[i])
    return m.done()


def difluoroethene(z):
    m = Builder()
    a = m.atom(C, (-0.65, 0, 0))
    b = m.atom(C, (0.65, 0, 0), a, 2)
    m.atom(F, (-1.3, 1.1, 0), a)
    m.atom(H, (-1.3, -1.1, 0), a)
    m.atom(F, (1.3, 1.1 if z else -1.1, 0), b)
    m.atom(H, (1.3, -1.1 if z else 1.1, 0), b)
    return m.done()


def acetaldoxime(z):
    """CH3-CH=N-OH: a C=N site whose nitrogen has one substituent."""
    m = Builder()
    c = m.atom(C, (-0.65, 0, 0))
    n = m.atom(N, (0.65, 0, 0), c, 2)
    me = m.atom(C, (-1.3, 1.1, 0), c)
    m.atom(H, (-1.3, -1.1, 0), c)
    o = m.atom(O, (1.3, 1.1 if z else -1.1, 0), n)
    m.atom(H, (2.2, 1.1 if z else -1.1, 0), o)
    for d in ((-0.5, 0.6, 0.9), (-0.5, 0.6, -0.9), (-1.0, 0.9, 0.0)):
        m.atom(H, np.asarray((-1.3, 1.1, 0)) + d, me)
    return m.done()


def methane():
    m = Builder()
    c = m.atom(C, (0, 0, 0))
    for k in range(4):
        m.atom(H, T[k] * 1.1, c)
    return m.done()


def neopentane():
    m = Builder()
    c = m.atom(C, (0, 0, 0))
    for k in range(4):
        m.methyl(T[k] * 1.5, c, 1, k)
    return m.done()


def cubane():
    m = Builder()
    corners = [np.array([(i >> 2 & 1) * 2 - 1, (i >> 1 & 1) * 2 - 1, (i & 1) * 2 - 1], float) for i in range(8)]
    c = [m.atom(C, p * 0.78) for p in corners]
    for i in range(8):
        for b in (1, 2, 4):
            if i < i ^ b:
                m.bond(c[i], c[i ^ b])
    for i in range(8):
        m.atom(H, corners[i] * 1.41, c[i])
    return m.done()


def difluoroallene():
    """F-CH=C=CH-F: the two end planes are perpendicular, the molecule is chiral - and has no site (the stated deviation)."""
    m = Builder()
    a = m.atom(C, (-1.3, 0, 0))
    mid = m.atom(C, (0, 0, 0), a, 2)
    b = m.atom(C, (1.3, 0, 0), mid, 2)
    m.atom(F, (-1.9, 1.0, 0), a)
    m.atom(H, (-1.9, -1.0, 0), a)
    m.atom(F, (1.9, 0, 1.0), b)
    m.atom(H, (1.9, 0, -1.0), b)
    return m.done()


def hand_table():
    """[(name, generated, ground truth, (isomorphisms, same, mirror) or None, verdict)]: the table of the issue that introduced the metric."""
    fe, chiral, meso = fluoroethanol(), difluorobutane(False), difluorobutane(True)
    cis, trans, z, e = difluorocyclobutane(True), difluorocyclobutane(False), difluoroethene(True), difluoroethene(False)
    return [
        ("1-fluoroethanol / itself", fe, fe, (1, 1, 0), IDENTICAL),
        ("1-fluoroethanol / mirror image", fe, reflected(fe), (1, 0, 1), MIRROR),
        ("chiral 2,3-difluorobutane / itself", chiral, chiral, (2, 2, 0), IDENTICAL),
        ("chiral 2,3-difluorobutane / enantiomer", chiral, reflected(chiral), (2, 0, 2), MIRROR),
        ("chiral 2,3-difluorobutane / meso", chiral, meso, (2, 0, 0), STEREOISOMER),
        ("meso 2,3-difluorobutane / itself", meso, meso, (2, 1, 1), IDENTICAL),
        ("meso 2,3-difluorobutane / mirror image", meso, reflected(meso), (2, 1, 1), IDENTICAL),
        ("cis-1,3-difluorocyclobutane / itself", cis, cis, (4, 2, 2), IDENTICAL),
        ("cis- / trans-1,3-difluorocyclobutane", cis, trans, (4, 0, 0), STEREOISOMER),
        ("cis-1,3-difluorocyclobutane / mirror image", cis, reflected(cis), None, IDENTICAL),
        ("trans-1,3-difluorocyclobutane / mirror image", trans, reflected(trans), None, IDENTICAL),
        ("(Z)-1,2-difluoroethene / itself", z, z, (2, 2, 0), IDENTICAL),
        ("(Z)- / (E)-1,2-difluoroethene", z, e, (2, 0, 0), STEREOISOMER),
        ("(Z)-1,2-difluoroethene / mirror image", z, reflected(z), (2, 2, 0), IDENTICAL),
        ("acetaldoxime / same isomer", acetaldoxime(True), acetaldoxime(True), (1, 1, 0), IDENTICAL),
        ("acetaldoxime / other isomer", acetaldoxime(True), acetaldoxime(False), (1, 0, 0), STEREOISOMER),
        ("methane", methane(), methane(), (1, 1, 0), IDENTICAL),
        ("neopentane", neopentane(), neopentane(), (24, 12, 12), IDENTICAL),
        ("cubane", cubane(), cubane(), (48, 24, 24), IDENTICAL),
        ("1,3-difluoroallene / mirror image", difluoroallene(), reflected(difluoroallene()), None, IDENTICAL),
        ("flattened 1-fluoroethanol", fluoroethanol(flat=True), fe, None, UNASSIGNED),
        ("1-fluoroethanol / C=O", fluoroethanol(double_co=True), fe, None, DIFFERENT),
    ]


# ------------------------------------------------------------------------------------------------------------------ the seeded pair set

SEEDS = (20261029, 20261033, 20261036)    # chosen so that the set holds every verdict 0, 1, 4, 5, 6 and no |V| or |c| within 1e-6 of its threshold
SIZES = tuple(range(1, 13)) + (29,)


def _gaussian(mol, rng):
    """The graph of ``mol`` with Gaussian positions (fp32 values)."""
    n = len(mol["type"])
    return dict(pos=_f32(rng.normal(size=(n, 3)) * 1.5), type=mol["type"], fc=mol["fc"], bond=mol["bond"])


def _first_centre(mol):
    p = perceive(mol)
    return (p["tetra"][0]["nbrs"][0], p["tetra"][0]["nbrs"][1]) if p["tetra"] else None


@functools.lru_cache(maxsize=2)
def seeded_pairs(seeds=SEEDS):
    """(generated molecules, ground truths, treatment names): for every seed and every n of SIZES a ``graph_mirror.random_molecule`` with
    Gaussian positions as the ground truth, and as the generated side: the same molecule, it renumbered and moved, its mirror image (renumbered),
    it with two neighbours of its first centre exchanged (renumbered; the plain copy where it has no centre), and the four bond edits of
    ``graph_mirror.treated`` (whose positions are fresh, so their centres are unrelated to the ground truth's)."""
    prb, ref, names = [], [], []
    for seed in seeds:
        rng = np.random.default_rng(seed)
        for n in SIZES:
            gt = _gaussian(GM.random_molecule(rng, n), rng)
            pair = _first_centre(gt)
            made = [("identity", gt), ("moved", renumbered(gt, rng)), ("reflected", renumbered(reflected(gt), rng)),
                    ("swapped", renumbered(neighbours_swapped(gt, *pair), rng) if pair else gt)]
            for kind in range(4 if n > 1 else 1):          # a single atom has no bond to edit and no second atom to swap types with
                t = GM.treated(gt, kind, rng)
                t["pos"] = _f32(t["pos"])
                made.append((f"treated {kind}", t))
            for name, mol in made:
                prb.append(mol)
                ref.append(gt)
                names.append(f"{seed}/{n}/{name}")
    return prb, ref, names


@functools.lru_cache(maxsize=2)
def seeded_results(seeds=SEEDS):
    """``compare`` of every seeded pair, computed once and shared."""
    prb, ref, _ = seeded_pairs(seeds)
    return [compare(a, b) for a, b in zip(prb, ref)]
