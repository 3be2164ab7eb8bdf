"""CPU yardstick of ``dsi_key_sites``, ``dsi_key_identity_records`` and ``key_identity_batch`` (include/diffspectra_key.h) in plain Python
and numpy float64, written from the header and not from the kernels.  Normal forms come from ``tests/mobile_mirror.py``; the bonds on shift
paths from its brute-force enumeration of every simple path over every neighbour (``Analysis.paths``); ring bonds from a reachability walk
without the bond; twins from ``stereo_mirror.twins_of`` on the normal form; isomorphisms of normal forms from ``stereo_mirror.isomorphisms``
(textbook backtracking, no refinement); and every isomorphism is tested against the sites by GEOMETRY, as ``stereo_mirror.compare`` does: the
volume of the ground truth's centre recomputed with its neighbours (and its hydrogen slot) in the order of the images, the cis bit of the
image substituents read off their own cosine.  The kernel does both in integers (parity of the images, flips from the lowest substituent),
so an agreement of the two is evidence for both.

All of this restates InChI as remembered and is UNPINNED against InChI.  Also here: the hand-stated table and the seeded sets the CPU and
the GPU tests share.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import graph_mirror as GM, mobile_mirror as MM, stereo_mirror as ST, structure_mirror as SM, valence_mirror as VM

W = SM.W
DIFFERENT, IDENTICAL, UNDECIDED, INVALID, MIRROR, STEREOISOMER, UNASSIGNED = range(7)
OK, ROW_UNDECIDED, UNUSABLE, OVERFLOW = MM.OK, MM.UNDECIDED, MM.UNUSABLE, MM.OVERFLOW
KIND_CENTRE, KIND_END, ASSIGNED, SIGN, HSLOT, NO_PARTNER = 1, 2, 4, 8, 16, 255
MASKS = ("tetra_site", "tetra_assigned", "tetra_positive", "ez_site", "ez_assigned", "ez_cis", "twin", "mobile_bond", "ring_bond")
MIN_VOLUME = MIN_PLANARITY = 0.5
DEFAULT_NODES = MM.DEFAULT_NODES
H, C, N, O, F = range(5)


# ------------------------------------------------------------------------------------------------------------------ perception

def _ring_bond(order, a, b):
    """Is the bond a-b a ring bond: b is reached from a without it, over the bonds of any order of the original record."""
    seen, todo = {a}, [a]
    while todo:
        u = todo.pop()
        for v in range(len(order)):
            if order[u][v] and v not in seen and {u, v} != {a, b}:
                seen.add(v)
                todo.append(v)
    return b in seen


def _site_nodes(A):
    """Nodes of the site search: every extension of rule 6 of diffspectra_mobile.h over every donor, WITHOUT the early stop."""
    if not A.acceptors:
        return 0
    count = [0]

    def extend(u, onpath):
        for v in A.nbrs[u]:
            if A.orders[u][v] != 1 or v not in A.interior or v in onpath:
                continue
            count[0] += 1
            w = [j for j in A.nbrs[v] if A.orders[v][j] == 2][0]
            if w not in onpath and w in A.interior:
                extend(w, onpath | {v, w})
    for d in A.donors:
        extend(d, {d})
    return count[0]


class Perception:
    """One molecule at the level of include/diffspectra_key.h.  ``status``; when it is OK: ``nf`` (the normal form as a molecule dict),
    ``source`` (original atom of every kept node), ``ordinal`` / ``twin`` per node, ``hatom`` {node: original hydrogen behind its slot},
    ``tetra`` = [dict(atom, nbrs, h, pts, V, assigned, positive)] and ``ez`` = [dict(a, b, subs_a, subs_b, pts_a, pts_b, assigned, cis)]
    (a < b; nodes in normal-form indices, ``None`` for the hydrogen slot, always last; ``pts``: the same as original atoms), ``mobile`` /
    ``ring`` = the nodes at the ends of the rejected double bonds, ``nodes``, ``margin``."""

    def __init__(self, mol, max_nodes=DEFAULT_NODES, min_volume=MIN_VOLUME, min_planarity=MIN_PLANARITY):
        rec, n = SM.records([mol])
        A = MM.Analysis(rec[0], n[0], max_nodes)
        self.status, self.nodes, self.tetra, self.ez, self.margin = A.status, 0, [], [], np.inf
        self.mobile, self.ring, self.hatom, self.twin, self.ordinal, self.total = set(), set(), {}, [], [], 0
        if A.status != OK:
            return
        nodes = _site_nodes(A)
        if nodes > max_nodes:
            self.status = ROW_UNDECIDED
            return
        out, total, source, status = MM.normal_row(rec[0], n[0], max_nodes, found=A)
        if status != OK:
            self.status = status
            return
        self.nodes, self.total, self.source = nodes, total, [s for s in source[:total]]
        self.nf = SM.mol_from_record(out, total)
        pos = np.asarray(mol["pos"], np.float64)
        slot = {a: r for r, a in enumerate(A.kept)}
        are_twins, self.ordinal, self.twin = ST.twins_of(self.nf)
        no_twins = lambda atoms: not any(are_twins(slot[i], slot[j]) for i in atoms for j in atoms)
        moved = {i for i in A.kept if VM.applied_charge(A.types[i], A.raw[i]) != A.q_res[i]}
        excluded = set(A.group_of) | moved
        folded = {i: [j for j in range(A.n) if A.orders[i][j] and j not in slot] for i in A.kept}
        hatom = {i: folded[i][0] for i in A.kept if i not in excluded and A.fixed[i] == 1 and len(folded[i]) == 1}
        self.hatom = {slot[i]: h for i, h in hatom.items()}
        double = [(a, b) for a in A.kept for b in A.kept if a < b and A.orders[a][b] == 2]
        on_path = {frozenset(path[k:k + 2]) for path in A.paths for k in range(len(path) - 1) if A.orders[path[k]][path[k + 1]] == 2}
        in_ring = {frozenset(ab) for ab in double if _ring_bond(A.orders, *ab)}
        self.mobile = {slot[x] for ab in double if frozenset(ab) in on_path for x in ab}
        self.ring = {slot[x] for ab in double if frozenset(ab) in in_ring for x in ab}

        for a in A.kept:
            nb = A.nbrs[a]
            if a in excluded or len(nb) + (a in hatom) != 4 or not no_twins(nb):
                continue
            pts = nb + ([hatom[a]] if a in hatom else [])
            V = ST.volume(pos, a, pts)
            if np.isfinite(V):
                self.margin = min(self.margin, abs(abs(V) - min_volume))
            assigned = bool(np.isfinite(pos[[a] + pts]).all() and abs(V) >= min_volume)
            self.tetra.append(dict(atom=slot[a], nbrs=[slot[j] for j in nb], h=a in hatom, centre=a, pts=pts, V=V, assigned=assigned,
                                   positive=bool(assigned and V > 0)))

        def end(a, b):
            if a in excluded or any(A.orders[a][j] >= 2 for j in range(A.n) if j != b):
                return None
            subs = [j for j in A.nbrs[a] if j != b]
            return subs + ([hatom[a]] if a in hatom else []) if len(subs) + (a in hatom) in (1, 2) and no_twins(subs) else None

        for a, b in double:
            if frozenset((a, b)) in on_path or frozenset((a, b)) in in_ring:
                continue
            pa, pb = end(a, b), end(b, a)
            if pa is None or pb is None:
                continue
            good, cis = True, {}
            for s in pa:
                for t in pb:
                    c, usable = ST.cosine(pos, a, b, s, t)
                    if np.isfinite(c):
                        self.margin = min(self.margin, abs(abs(c) - min_planarity))
                    good = good and usable and abs(c) >= min_planarity
                    cis[s, t] = c > 0
            if len(pa) == 2:
                good = good and all(cis[pa[0], t] != cis[pa[1], t] for t in pb)
            if len(pb) == 2:
                good = good and all(cis[s, pb[0]] != cis[s, pb[1]] for s in pa)
            self.ez.append(dict(a=slot[a], b=slot[b], ends=(a, b), subs_a=[slot.get(j) for j in pa], subs_b=[slot.get(j) for j in pb], pts_a=pa, pts_b=pb,
                                assigned=bool(good), cis=bool(good and cis[pa[0], pb[0]])))
        self.margin = float(self.margin)

    @property
    def open(self):
        return sum(not s["assigned"] for s in self.tetra) + sum(not s["assigned"] for s in self.ez)


def site_rows(mol, max_nodes=DEFAULT_NODES, min_volume=MIN_VOLUME, min_planarity=MIN_PLANARITY, found=None):
    """What ``dsi_key_sites`` writes for one record: dict(site [29, 2], masks [9], volume [29], nodes, status)."""
    P = Perception(mol, max_nodes, min_volume, min_planarity) if found is None else found
    site, vol = np.zeros((W, 2), np.uint8), np.zeros(W)
    site[:, 1] = NO_PARTNER
    if P.status != OK:
        return dict(site=site, masks=[0] * 9, volume=vol, nodes=0, status=P.status)
    bits = lambda atoms: sum(1 << a for a in set(atoms))
    for a in P.hatom:
        site[a, 0] |= HSLOT
    for s in P.tetra:
        site[s["atom"], 0] |= KIND_CENTRE | (ASSIGNED if s["assigned"] else 0) | (SIGN if s["positive"] else 0)
        vol[s["atom"]] = s["V"]
    for s in P.ez:
        for x, y in ((s["a"], s["b"]), (s["b"], s["a"])):
            site[x, 0] |= KIND_END | (ASSIGNED if s["assigned"] else 0) | (SIGN if s["cis"] else 0)
            site[x, 1] = y
    ends = lambda key: [x for s in P.ez if key is None or s[key] for x in (s["a"], s["b"])]
    masks = [bits(s["atom"] for s in P.tetra), bits(s["atom"] for s in P.tetra if s["assigned"]), bits(s["atom"] for s in P.tetra if s["positive"]),
             bits(ends(None)), bits(ends("assigned")), bits(ends("cis")), bits(i for i in range(P.total) if P.twin[i]), bits(P.mobile), bits(P.ring)]
    return dict(site=site, masks=masks, volume=vol, nodes=P.nodes, status=OK)


# ------------------------------------------------------------------------------------------------------------------ comparison

def kind_of(b, pa, pb, image):
    """What the isomorphism ``image`` of the normal forms does to the sites (``pa`` / ``pb``: ``Perception`` of both molecules, every site
    assigned; ``b``: the ground truth's ORIGINAL molecule): 'same', 'mirror' or 'other'.  Sites onto sites first, as the header states it;
    then the geometry of ``b`` under the images."""
    centre_b = {s["atom"]: s for s in pb.tetra}
    bond_b = {frozenset((s["a"], s["b"])): s for s in pb.ez}
    hslot = lambda p, x: x in p.hatom
    if len(pa.tetra) != len(pb.tetra) or len(pa.ez) != len(pb.ez):
        return "other"
    for s in pa.tetra:
        if image[s["atom"]] not in centre_b or hslot(pa, s["atom"]) != hslot(pb, image[s["atom"]]):
            return "other"
    for s in pa.ez:
        if frozenset((image[s["a"]], image[s["b"]])) not in bond_b or any(hslot(pa, x) != hslot(pb, image[x]) for x in (s["a"], s["b"])):
            return "other"
    pos = np.asarray(b["pos"], np.float64)
    origin = lambda node: pb.source[node]                             # original atom of a kept node of b
    point = lambda node, owner: origin(image[node]) if node is not None else pb.hatom[image[owner]]
    kept, turned = 0, 0
    for s in pa.tetra:
        order = [point(j, s["atom"]) for j in s["nbrs"]] + ([point(None, s["atom"])] if s["h"] else [])
        positive = ST.volume(pos, origin(image[s["atom"]]), order) > 0
        kept += positive == s["positive"]
        turned += positive != s["positive"]
    ez_kept = True
    for s in pa.ez:
        c, _ = ST.cosine(pos, origin(image[s["a"]]), origin(image[s["b"]]), point(s["subs_a"][0], s["a"]), point(s["subs_b"][0], s["b"]))
        ez_kept = ez_kept and (c > 0) == s["cis"]
    if turned == 0 and ez_kept:
        return "same"
    if pa.tetra and kept == 0 and ez_kept:
        return "mirror"
    return "other"


def compare(a, b, max_nodes=DEFAULT_NODES, min_volume=MIN_VOLUME, min_planarity=MIN_PLANARITY, pa=None, pb=None):
    """One pair, ``a`` the generated molecule and ``b`` the ground truth (ORIGINAL molecules), every search run to its end:
    dict(verdict, found [3], sites [4], margin, maps, status = (of a, of b)).  A side that is unusable gives INVALID, a side over a budget or
    over 29 nodes UNDECIDED - what ``key_identity_batch`` returns; found, sites and maps are then empty."""
    pa = Perception(a, max_nodes, min_volume, min_planarity) if pa is None else pa
    pb = Perception(b, max_nodes, min_volume, min_planarity) if pb is None else pb
    maps = dict(iso=[], same=[], mirror=[])
    if pa.status != OK or pb.status != OK:
        verdict = INVALID if UNUSABLE in (pa.status, pb.status) else UNDECIDED
        return dict(verdict=verdict, found=[0, 0, 0], sites=[0, 0, 0, 0], margin=np.inf, maps=maps, status=(pa.status, pb.status))
    sites = [len(pa.tetra), len(pa.ez), pa.open, pb.open]
    assigned = sites[2] + sites[3] == 0
    for image in ST.isomorphisms(pa.nf, pb.nf, pa.ordinal, pb.ordinal):
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
    return dict(verdict=verdict, found=[len(maps["iso"]), len(maps["same"]), len(maps["mirror"])], sites=sites, margin=min(pa.margin, pb.margin),
                maps=maps, status=(OK, OK))


def identity(a, b, max_nodes=DEFAULT_NODES):
    """(verdict, strict, layer) of ``key_identity_batch`` for the probe ``a`` and the ground truth ``b``."""
    strict = ST.compare(a, b)["verdict"]
    verdict = compare(a, b, max_nodes)["verdict"]
    return verdict, strict, (0 if strict == IDENTICAL else 1) if verdict == IDENTICAL else -1


def map_claim(a, b, image, verdict, pa=None, pb=None):
    """Does the normal-form map a kernel returned with ``verdict`` have the property the verdict claims?  An isomorphism of the normal forms
    that respects the ordinals for 1, 4, 5 and 6 - a same one for 1, a mirror one for 4 -, all -1 for every other verdict."""
    image = [int(x) for x in image]
    if verdict not in (IDENTICAL, MIRROR, STEREOISOMER, UNASSIGNED):
        return all(x == -1 for x in image)
    pa, pb = pa or Perception(a), pb or Perception(b)
    n = pa.total
    if any(x != -1 for x in image[n:]) or not GM.is_isomorphism(pa.nf, pb.nf, image[:n]):
        return False
    if any(pa.ordinal[i] != pb.ordinal[image[i]] for i in range(n)):
        return False
    if verdict in (IDENTICAL, MIRROR):
        return kind_of(b, pa, pb, image[:n]) == ("same" if verdict == IDENTICAL else "mirror")
    return True


def translated(pa, pb, image):
    """A normal-form map as ``key_identity_batch`` returns it: ground-truth ORIGINAL kept atom of every generated ORIGINAL kept atom."""
    out = [-1] * W
    for node, target in enumerate(image[:pa.total]):
        if target >= 0 and pa.source[node] != 0xff:
            out[pa.source[node]] = pb.source[target]
    return out


def plain(mol, max_nodes=DEFAULT_NODES):
    """No mobile group, no proton transfer, no ring double bond: the molecules on which this level must agree with ``stereo_mirror.compare``."""
    rec, n = SM.records([mol])
    A = MM.Analysis(rec[0], n[0], max_nodes)
    if A.status != OK:
        return False
    moved = any(VM.applied_charge(A.types[i], A.raw[i]) != A.q_res[i] for i in A.kept)
    ring = any(A.orders[a][b] == 2 and _ring_bond(A.orders, a, b) for a in range(A.n) for b in range(a + 1, A.n))
    return not A.groups and not moved and not ring


def within_valence(mol):
    """Chemically usable: a usable record none of whose atoms exceeds the valence of its element and applied charge.  Only then do the
    hydrogens of the normal form tell the bond orders of the drawing: an over-filled atom has no implicit hydrogen to lose."""
    rec, n = SM.records([mol])
    A = MM.Analysis(rec[0], n[0])
    return A.status == OK and all(sum(A.orders[i]) <= VM.VMAX[A.types[i], VM.applied_charge(A.types[i], A.raw[i])] for i in range(A.n))


def fold_made_twins(mol, found=None):
    """The pairs of kept atoms (original indices) that are twins on the normal form and not on the drawing: two NH2, OH or CH3 ... groups on
    one atom, leaves only once their hydrogens are folded.  A centre that carries such a pair is a site of diffspectra_stereo.h (its symmetry
    is found there as an automorphism) and none here."""
    P = found or Perception(mol)
    if P.status != OK:
        return []
    drawn, _, _ = ST.twins_of(mol)
    folded, _, _ = ST.twins_of(P.nf)
    kept = [(node, atom) for node, atom in enumerate(P.source) if atom != 0xff]
    return [(a, b) for i, a in kept for j, b in kept if i < j and folded(i, j) and not drawn(a, b)]


# ------------------------------------------------------------------------------------------------------------------ the hand table

T = ST.T
reflected = ST.reflected


class Builder(ST.Builder):
    """``stereo_mirror.Builder`` with formal charges."""

    def __init__(self):
        super().__init__()
        self.fc = {}

    def charge(self, atom, q):
        self.fc[atom] = q
        return atom

    def done(self):
        mol = super().done()
        for atom, q in self.fc.items():
            mol["fc"][atom] = q
        return mol


def _acid(m, at, bonded_to, h_on, out):
    """-C(=O)OH at ``at``, its oxygens towards ``out``; the hydrogen sits on oxygen ``h_on`` (0 or 1), the other one is the carbonyl."""
    at, out = np.asarray(at, float), np.asarray(out, float)
    side = np.cross(out, (0.3, 0.5, 0.8))
    side /= np.linalg.norm(side)
    c = m.atom(C, at, bonded_to)
    spots = [at + out * 0.6 + side * 1.05, at + out * 0.6 - side * 1.05]
    o = [m.atom(O, spots[k], c, 1 if k == h_on else 2) for k in range(2)]
    m.atom(H, spots[h_on] + out * 0.95, o[h_on])
    return c


def lactic_acid(h_on=0):
    """CH3-CH(OH)-COOH: one centre (atom 0) with a hydrogen slot; ``h_on`` names the acid oxygen that carries the hydrogen."""
    m = Builder()
    c = m.atom(C, (0, 0, 0))
    m.methyl(T[0] * 1.5, c, 1, 0)
    o = m.atom(O, T[1] * 1.4, c)
    m.atom(H, T[1] * 2.35, o)
    _acid(m, T[2] * 1.5, c, h_on, T[2])
    m.atom(H, T[3] * 1.1, c)
    return m.done()


def alanine(zwitterion=False):
    """CH3-CH(NH2)-COOH, or CH3-CH(NH3+)-COO-: one centre (atom 0) with a hydrogen slot."""
    m = Builder()
    c = m.atom(C, (0, 0, 0))
    m.methyl(T[0] * 1.5, c, 1, 0)
    n = m.atom(N, T[1] * 1.45, c)
    for k in range(3 if zwitterion else 2):
        m.atom(H, T[1] * 1.45 + T[1] * 0.4 + np.roll(T[1], 1) * (k - 1) * 0.9 + np.roll(T[1], 2) * (k % 2) * 0.8, n)
    if zwitterion:
        m.charge(n, 1)
        cc = m.atom(C, T[2] * 1.5, c)
        m.atom(O, T[2] * 2.1 + np.roll(T[2], 1) * 1.05, cc, 2)
        m.charge(m.atom(O, T[2] * 2.1 - np.roll(T[2], 1) * 1.05, cc), -1)
    else:
        _acid(m, T[2] * 1.5, c, 0, T[2])
    m.atom(H, T[3] * 1.1, c)
    return m.done()


def fluoroethylimidazole(five):
    """The imidazole N0 C1 N2 C3 C4 with CHF-CH3 on C3, ring atoms first: the 4-tautomer N0(H) C1=N2 (``five`` false) or the 5-tautomer N0=C1
    N2(H).  One centre (atom 5) outside the ring with a hydrogen slot; the ring's double bonds are ring bonds."""
    m = Builder()
    e = np.array((1.0, -1.0, 0.0)) / np.sqrt(2.0)                    # normal to T[0]: the ring lies in the plane of T[0] and e
    middle = T[0] * 2.65
    spot = lambda k, r: middle + r * (np.cos(np.radians(72.0 * (k - 3))) * -T[0] + np.sin(np.radians(72.0 * (k - 3))) * e)
    orders = [2, 1, 1, 2, 1] if five else [1, 2, 1, 2, 1]            # of the bonds 0-1, 1-2, 2-3, 3-4, 4-0
    ring = [m.atom(N if k in (0, 2) else C, spot(k, 1.15)) for k in range(5)]
    for k in range(5):
        m.bond(ring[k], ring[(k + 1) % 5], orders[k])
    c = m.atom(C, (0, 0, 0), ring[3])
    for k in (1, 4, 2 if five else 0):
        m.atom(H, spot(k, 2.2), ring[k])
    m.atom(F, T[1] * 1.4, c)
    m.methyl(T[2] * 1.5, c, 1, 2)
    m.atom(H, T[3] * 1.1, c)
    return m.done()


def _vinyl(m, left, right):
    """a=b along x in the plane z = 0; ``left`` / ``right``: callables (atom, spot above, spot below) that hang the substituents."""
    a = m.atom(C, (-0.65, 0, 0))
    b = m.atom(C, (0.65, 0, 0), a, 2)
    left(a, np.array((-1.3, 1.1, 0.0)), np.array((-1.3, -1.1, 0.0)))
    right(b, np.array((1.3, 1.1, 0.0)), np.array((1.3, -1.1, 0.0)))
    return a, b


def crotonic_acid(z, h_on=0):
    """CH3-CH=CH-COOH: methyl above on the left; the acid above (Z) or below (E) on the right; both ends have a hydrogen slot."""
    m = Builder()

    def left(a, up, down):
        m.methyl(up, a, 1, 0)
        m.atom(H, down, a)

    def right(b, up, down):
        spot, other = (up, down) if z else (down, up)
        _acid(m, spot, b, h_on, (spot - (0.65, 0, 0)) / np.linalg.norm(spot - (0.65, 0, 0)))
        m.atom(H, other, b)
    _vinyl(m, left, right)
    return m.done()


def butenedioic_acid(z, h_left, h_right):
    """HOOC-CH=CH-COOH: maleic (Z) or fumaric (E) acid, the acid hydrogens on the oxygens named."""
    m = Builder()

    def left(a, up, down):
        _acid(m, up, a, h_left, (up + (0.65, 0, 0)) / np.linalg.norm(up + (0.65, 0, 0)))
        m.atom(H, down, a)

    def right(b, up, down):
        spot, other = (up, down) if z else (down, up)
        _acid(m, spot, b, h_right, (spot - (0.65, 0, 0)) / np.linalg.norm(spot - (0.65, 0, 0)))
        m.atom(H, other, b)
    _vinyl(m, left, right)
    return m.done()


def methylacetimidic_acid(z):
    """CH3-C(OH)=N-CH3, atoms C0 N1 first: the C=N lies on the shift path from the OH."""
    m = Builder()
    c = m.atom(C, (-0.65, 0, 0))
    n = m.atom(N, (0.65, 0, 0), c, 2)
    m.methyl((-1.3, 1.1, 0), c, 1, 0)
    o = m.atom(O, (-1.3, -1.1, 0), c)
    m.atom(H, (-2.2, -1.2, 0), o)
    m.methyl((1.3, 1.1 if z else -1.1, 0), n, -1, 0)
    return m.done()


def methylacetamide():
    """CH3-C(=O)-NH-CH3 on the same skeleton, atoms C0 N1 first: the C=O lies on the shift path from the NH."""
    m = Builder()
    c = m.atom(C, (-0.65, 0, 0))
    n = m.atom(N, (0.65, 0, 0), c)
    m.methyl((-1.3, 1.1, 0), c, 1, 0)
    m.atom(O, (-1.3, -1.1, 0), c, 2)
    m.methyl((1.3, 1.1, 0), n, -1, 0)
    m.atom(H, (1.3, -1.1, 0), n)
    return m.done()


def hydroxyacrolein(z):
    """HO-CH=CH-CH=O, atoms C0 C1 first: both double bonds lie on the shift path between the oxygens."""
    m = Builder()

    def left(a, up, down):
        o = m.atom(O, up, a)
        m.atom(H, up + (-0.9, 0.2, 0), o)
        m.atom(H, down, a)

    def right(b, up, down):
        spot, other = (up, down) if z else (down, up)
        c = m.atom(C, spot, b)
        m.atom(O, spot + (1.2, 0.1, 0), c, 2)
        m.atom(H, spot + (-0.1, 1.0 if z else -1.0, 0), c)
        m.atom(H, other, b)
    _vinyl(m, left, right)
    return m.done()


def fluoroethanol_2():
    """F-CH2-CH2-OH: the atoms of 1-fluoroethanol on another skeleton."""
    m = Builder()
    c0 = m.atom(C, (0, 0, 0))
    c1 = m.atom(C, T[0] * 1.5, c0)
    m.atom(F, T[1] * 1.4, c0)
    o = m.atom(O, T[0] * 1.5 - T[1] * 1.4, c1)
    m.atom(H, T[0] * 1.5 - T[1] * 2.3, o)
    for at, c in ((T[2] * 1.1, c0), (T[3] * 1.1, c0), (T[0] * 1.5 - T[2] * 1.1, c1), (T[0] * 1.5 - T[3] * 1.1, c1)):
        m.atom(H, at, c)
    return m.done()


def flat(mol, heavy):
    """A molecule of ``mobile_mirror.hand_table`` (heavy atoms first, hydrogens behind them) with positions: the heavy atoms at ``heavy``, every
    hydrogen 1 A from its parent, away from the centroid and a little out of the plane."""
    heavy = np.asarray(heavy, float)
    n, k = len(mol["type"]), len(heavy)
    pos, middle = np.zeros((n, 3)), heavy.mean(axis=0)
    pos[:k] = heavy
    bond = np.asarray(mol["bond"])
    for h in range(k, n):
        parent = int(np.nonzero(bond[h] + bond[:, h])[0][0])
        out = heavy[parent] - middle
        pos[h] = heavy[parent] + out / max(np.linalg.norm(out), 1e-9) + (0, 0, 0.35 * (h - k - 1))
    return dict(pos=ST._f32(pos), type=mol["type"], fc=mol["fc"], bond=mol["bond"])


def _hexagon(*extra):
    ring = [(1.39 * np.cos(np.radians(60.0 * k)), 1.39 * np.sin(np.radians(60.0 * k)), 0.0) for k in range(6)]
    return ring + [tuple(2.8 / 1.39 * np.asarray(ring[k])) for k in extra]


def hand_molecules():
    """{name: molecule} of the table below."""
    named = {name: mol for name, mol, _ in MM.hand_table()}
    fe = ST.fluoroethanol()
    out = {
        "lactic acid": lactic_acid(0), "lactic acid, the other oxygen": lactic_acid(1),
        "alanine": alanine(False), "alanine zwitterion": alanine(True),
        "4-(1-fluoroethyl)imidazole": fluoroethylimidazole(False), "5-(1-fluoroethyl)imidazole": fluoroethylimidazole(True),
        "(E)-crotonic acid": crotonic_acid(False, 0), "(E)-crotonic acid, the other oxygen": crotonic_acid(False, 1), "(Z)-crotonic acid": crotonic_acid(True, 0),
        "(E)-N-methylacetimidic acid": methylacetimidic_acid(False), "(Z)-N-methylacetimidic acid": methylacetimidic_acid(True),
        "N-methylacetamide": methylacetamide(),
        "(E)-3-hydroxyacrolein": hydroxyacrolein(False), "(Z)-3-hydroxyacrolein": hydroxyacrolein(True),
        "(E)-acetaldoxime": ST.acetaldoxime(False), "(Z)-acetaldoxime": ST.acetaldoxime(True),
        "2-pyridone": flat(named["2-pyridone"], _hexagon(1)),
        "2-hydroxypyridine, N=C(OH)": flat(named["2-hydroxypyridine, N=C(OH)"], _hexagon(1)),
        "2-hydroxypyridine, N-C(OH)": flat(named["2-hydroxypyridine, N-C(OH)"], _hexagon(1)),
        "o-xylene, C1=C2": flat(named["o-xylene, C1=C2"], _hexagon(0, 1)), "o-xylene, C1-C2": flat(named["o-xylene, C1-C2"], _hexagon(0, 1)),
        "(Z)-1,2-difluoroethene": ST.difluoroethene(True), "(E)-1,2-difluoroethene": ST.difluoroethene(False),
        "fumaric acid": butenedioic_acid(False, 0, 1), "maleic acid": butenedioic_acid(True, 1, 0),
        "1-fluoroethanol": fe, "flattened 1-fluoroethanol": ST.fluoroethanol(flat=True), "1-fluoroethanol, C=O": ST.fluoroethanol(double_co=True),
        "1,3-difluoroallene": ST.difluoroallene(), "2-fluoroethanol": fluoroethanol_2(),
    }
    for name in [k for k in out if k.split(" ")[0] in ("lactic", "alanine", "4-(1-fluoroethyl)imidazole", "5-(1-fluoroethyl)imidazole", "1,3-difluoroallene")]:
        out[name + ", mirror image"] = reflected(out[name])
    return out


def hand_pairs():
    """[(generated, ground truth, verdict, layer or None)] by name, stated by hand from the header.  ``layer`` None: not stated.  The two
    drawings of an acid are ONE labelled graph as drawn (the oxygens change places, as in ``mobile_mirror.hand_pairs``), so such a pair has
    layer 0 by the definition of ``layer`` (0 whenever the strict verdict is identical); layer 1 needs drawings that differ as graphs."""
    I, M_, S_, U, D = IDENTICAL, MIRROR, STEREOISOMER, UNASSIGNED, DIFFERENT
    return [
        ("lactic acid", "lactic acid, the other oxygen", I, 0),
        ("lactic acid", "lactic acid, the other oxygen, mirror image", M_, -1),
        ("alanine", "alanine zwitterion", I, 1),
        ("alanine", "alanine zwitterion, mirror image", M_, -1),
        ("alanine zwitterion", "alanine", I, 1),
        ("4-(1-fluoroethyl)imidazole", "5-(1-fluoroethyl)imidazole", I, 1),
        ("4-(1-fluoroethyl)imidazole", "5-(1-fluoroethyl)imidazole, mirror image", M_, -1),
        ("(E)-crotonic acid", "(E)-crotonic acid", I, 0),
        ("(E)-crotonic acid", "(E)-crotonic acid, the other oxygen", I, 0),
        ("(E)-crotonic acid", "(Z)-crotonic acid", S_, -1),
        ("(E)-crotonic acid, the other oxygen", "(Z)-crotonic acid", S_, -1),
        ("(E)-N-methylacetimidic acid", "(Z)-N-methylacetimidic acid", I, 1),
        ("(E)-N-methylacetimidic acid", "N-methylacetamide", I, 1),
        ("(Z)-N-methylacetimidic acid", "N-methylacetamide", I, 1),
        ("N-methylacetamide", "(E)-N-methylacetimidic acid", I, 1),
        ("(E)-3-hydroxyacrolein", "(Z)-3-hydroxyacrolein", I, 1),
        ("(E)-acetaldoxime", "(Z)-acetaldoxime", S_, -1),
        ("(Z)-acetaldoxime", "(Z)-acetaldoxime", I, 0),
        ("2-pyridone", "2-hydroxypyridine, N=C(OH)", I, 1),
        ("2-pyridone", "2-hydroxypyridine, N-C(OH)", I, 1),
        ("2-hydroxypyridine, N=C(OH)", "2-hydroxypyridine, N-C(OH)", I, 1),
        ("o-xylene, C1=C2", "o-xylene, C1-C2", I, 1),
        ("(Z)-1,2-difluoroethene", "(E)-1,2-difluoroethene", S_, -1),
        ("fumaric acid", "maleic acid", S_, -1),
        ("fumaric acid", "fumaric acid", I, 0),
        ("flattened 1-fluoroethanol", "1-fluoroethanol", U, -1),
        ("1,3-difluoroallene", "1,3-difluoroallene, mirror image", I, None),
        ("2-fluoroethanol", "1-fluoroethanol", D, -1),                 # a changed skeleton
        # CH3-CHF-O(H)= with the C-O bond drawn double: a bond-order edit on an over-filled oxygen changes no hydrogen count, and the normal
        # form compares no bond orders - DIFFERENT as drawn (the table of stereo_mirror), the same molecule at this level
        ("1-fluoroethanol, C=O", "1-fluoroethanol", I, 1),
    ]


def hand_sites():
    """{name: dict(centres, hslots, ez, mobile, ring)} stated by hand, in ORIGINAL atom indices (every named atom is a kept atom): the
    centres, the atoms with a hydrogen slot that are a centre or an end, the E/Z site bonds, and the atoms at the ends of the double bonds
    rejected as mobile / as ring bonds."""
    row = lambda centres=(), hslots=(), ez=(), mobile=(), ring=(): dict(centres=set(centres), hslots=set(hslots), ez={frozenset(b) for b in ez},
                                                                        mobile=set(mobile), ring=set(ring))
    return {
        # C0; methyl C1 H2-4; O5 H6; acid C7 O8 O9 (H10); H11: the carbonyl lies on the path O-C=O
        "lactic acid": row([0], [0], mobile=[7, 9]),
        "lactic acid, the other oxygen": row([0], [0], mobile=[7, 8]),
        "alanine": row([0], [0], mobile=[8, 10]),
        "alanine zwitterion": row([0], [0], mobile=[9, 10]),
        # ring N0 C1 N2 C3 C4, centre C5: C1=N2 lies on the path N0-C1=N2 and is a ring bond, C3=C4 is a ring bond only
        "4-(1-fluoroethyl)imidazole": row([5], [5], mobile=[1, 2], ring=[1, 2, 3, 4]),
        "5-(1-fluoroethyl)imidazole": row([5], [5], mobile=[0, 1], ring=[0, 1, 3, 4]),
        # C0=C1; methyl C2; H6; acid C7 O8 O9
        "(E)-crotonic acid": row(hslots=[0, 1], ez=[(0, 1)], mobile=[7, 9]),
        "(E)-crotonic acid, the other oxygen": row(hslots=[0, 1], ez=[(0, 1)], mobile=[7, 8]),
        "(Z)-crotonic acid": row(hslots=[0, 1], ez=[(0, 1)], mobile=[7, 9]),
        "(E)-N-methylacetimidic acid": row(mobile=[0, 1]),
        "(Z)-N-methylacetimidic acid": row(mobile=[0, 1]),
        "N-methylacetamide": row(mobile=[0, 6]),
        # C0=C1; O2; C5=O6
        "(E)-3-hydroxyacrolein": row(mobile=[0, 1, 5, 6]),
        "(Z)-3-hydroxyacrolein": row(mobile=[0, 1, 5, 6]),
        "(E)-acetaldoxime": row(hslots=[0], ez=[(0, 1)]),
        "(Z)-acetaldoxime": row(hslots=[0], ez=[(0, 1)]),
        # N0 C1(O6) C2 C3 C4 C5
        "2-pyridone": row(mobile=[1, 2, 3, 4, 5, 6], ring=[2, 3, 4, 5]),
        "2-hydroxypyridine, N=C(OH)": row(mobile=[0, 1], ring=[0, 1, 2, 3, 4, 5]),
        "2-hydroxypyridine, N-C(OH)": row(mobile=[0, 1, 2, 3, 4, 5], ring=[0, 1, 2, 3, 4, 5]),
        "o-xylene, C1=C2": row(ring=[0, 1, 2, 3, 4, 5]),
        "o-xylene, C1-C2": row(ring=[0, 1, 2, 3, 4, 5]),
        "(Z)-1,2-difluoroethene": row(hslots=[0, 1], ez=[(0, 1)]),
        "(E)-1,2-difluoroethene": row(hslots=[0, 1], ez=[(0, 1)]),
        # C0=C1; left acid C2 O3 O4 (H5), H6; right acid C7 O8 O9
        "fumaric acid": row(hslots=[0, 1], ez=[(0, 1)], mobile=[2, 4, 7, 8]),
        "maleic acid": row(hslots=[0, 1], ez=[(0, 1)], mobile=[2, 3, 7, 9]),
        "1-fluoroethanol": row([0], [0]),
        "1,3-difluoroallene": row(),
    }


def stereo_table_pairs():
    """The pairs of ``stereo_mirror.hand_table()`` whose drawings have no mobile group and no ring double bond: (name, generated, ground
    truth, verdict stated there)."""
    return [(name, a, b, verdict) for name, a, b, _, verdict in ST.hand_table() if plain(a) and plain(b)]


# ------------------------------------------------------------------------------------------------------------------ the seeded sets

CORPUS_SEED = 20261021        # of mobile_mirror.corpus: see tests/test_key_identity_cpu.py for the conditions it was chosen under
POSITION_SEED = 20261101
MAX_DRAWS = 200


@functools.lru_cache(maxsize=1)
def corpus():
    """``mobile_mirror.corpus()`` with Gaussian positions (fp32 values)."""
    rng = np.random.default_rng(POSITION_SEED)
    return [ST._gaussian(m, rng) for m in MM.corpus(CORPUS_SEED)]


@functools.lru_cache(maxsize=1)
def law2_pairs():
    """(generated, ground truth, name) on which this level must agree with ``stereo_mirror.compare``: the pairs of
    ``stereo_mirror.seeded_pairs()`` with two plain records within their valences, and every plain molecule of ``corpus()`` against itself moved and
    renumbered, against its mirror image, against itself with two neighbours of its first centre exchanged and, every fourth, against another
    molecule of the corpus; a molecule with two centres or more is drawn again with fresh Gaussian positions until all its sites are assigned
    (MAX_DRAWS times at the most) and goes against itself with two neighbours of its first centre exchanged."""
    prb, ref, names = [], [], []
    for a, b, name in zip(*ST.seeded_pairs()):
        if within_valence(a) and within_valence(b) and plain(a) and plain(b):
            prb.append(a), ref.append(b), names.append("seeded " + name)
    rng = np.random.default_rng(POSITION_SEED + 1)
    for k, m in enumerate(corpus()):
        if not plain(m):
            continue
        pair = ST._first_centre(m)
        made = [("moved", ST.renumbered(m, rng)), ("reflected", ST.renumbered(reflected(m), rng))]
        if pair:
            made.append(("swapped", ST.renumbered(ST.neighbours_swapped(m, *pair), rng)))
        if k % 4 == 0:                                                # another molecule of the corpus: a different skeleton, or by chance the same
            other = corpus()[(k + 3) % len(corpus())]
            if plain(other):
                made.append(("other", ST.renumbered(other, rng)))
        for name, t in made:
            prb.append(t), ref.append(m), names.append(f"corpus {k} {name}")
        sites = ST.perceive(m)
        if len(sites["tetra"]) >= 2:                                  # another stereoisomer needs two sites, all of them assigned: a few per cent of
            for draw in range(MAX_DRAWS):                             # the Gaussian draws.  Such a molecule is drawn again until one is (seeds chosen
                again = ST._gaussian(m, rng)                          # on the CPU, by the mirror of diffspectra_stereo.h alone)
                drawn = ST.perceive(again)
                if all(s["assigned"] for s in drawn["tetra"] + drawn["ez"]):
                    prb.append(ST.renumbered(ST.neighbours_swapped(again, *pair), rng)), ref.append(again), names.append(f"corpus {k} swapped, draw {draw}")
                    break
    return prb, ref, names


@functools.lru_cache(maxsize=1)
def shifted_forms():
    """[(k, path, m, s)]: every molecule m of ``corpus()`` and every single ``mobile_mirror.shifted`` form s of it (positions kept)."""
    out = []
    for k, m in enumerate(corpus()):
        rec, n = SM.records([m])
        A = MM.Analysis(rec[0], n[0])
        if A.status != OK:
            continue
        for path in A.paths:
            s = MM.shifted(m, path)
            if s is not None:
                out.append((k, path, m, s))
    return out
