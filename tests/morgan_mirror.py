"""CPU yardstick of ``ds_morgan_records`` and ``ds_morgan_similarity_records`` (include/diffspectra_hip.h), in plain Python, written from
the header's definition term by term: kept atoms and bonds, the atom invariant (type, charge, kept degree, hydrogen count, cycle flag), the
iteration, the environments as literal sets of bonds, and the order-free duplicate-environment rule.  Nothing here is shaped like the kernel:
a bond set is a ``frozenset`` of atom pairs, the cycle flag removes a bond and walks the graph, and a fingerprint is a Python ``set`` of
ints.  A molecule is the dict of ``structure_mirror.mol_from_record`` (``type [n], fc [n], bond [n, n]``; ``pos`` is never read; bond bytes
come from the upper triangle).  Inputs of the tests: ``mces_mirror.seeded_pairs`` / ``random_molecule``.  Also here: the hand table.
"""
from __future__ import annotations

import numpy as np

from tests import graph_mirror as GM

MASK = GM.MASK
mix = GM.mix
MAX_RADIUS = 3


def kept_graph(mol, drop_h=True):
    """(kept atoms [original indices], {atom: {kept neighbour: bond byte}}, {atom: number of bonded neighbours of type 0, or 0})."""
    n = min(len(mol["type"]), GM.W)
    t = [int(x) & 255 for x in np.asarray(mol["type"])[:n]]
    b = np.asarray(mol["bond"]).astype(np.int64) & 255
    order = lambda i, j: int(b[min(i, j), max(i, j)])
    kept = [i for i in range(n) if not (drop_h and t[i] == 0)]
    nbr = {i: {j: order(i, j) for j in kept if j != i and order(i, j) > 0} for i in kept}
    hyd = {i: sum(1 for j in range(n) if j != i and t[j] == 0 and order(i, j) > 0) if drop_h else 0 for i in kept}
    return kept, nbr, hyd


def _connected_without(nbr, a, b):
    """Do a and b stay connected when the bond a-b is removed?"""
    seen, stack = {a}, [a]
    while stack:
        v = stack.pop()
        for u in nbr[v]:
            if {v, u} == {a, b} or u in seen:
                continue
            if u == b:
                return True
            seen.add(u)
            stack.append(u)
    return False


def atom_invariants(mol, drop_h=True):
    """{kept atom: id_0}."""
    kept, nbr, hyd = kept_graph(mol, drop_h)
    out = {}
    for i in kept:
        cyc = int(any(_connected_without(nbr, i, j) for j in nbr[i]))
        x = mix(int(mol["type"][i]) & 255, int(mol["fc"][i]) & 255)
        for term in (len(nbr[i]), hyd[i], cyc):
            x = mix(x, term)
        out[i] = x
    return out


def fingerprint(mol, drop_h=True, radius=2):
    """The set F_0 | ... | F_R of the header, as Python ints in [0, 2^64)."""
    assert 0 <= radius <= MAX_RADIUS
    kept, nbr, _ = kept_graph(mol, drop_h)
    ident = atom_invariants(mol, drop_h)
    features = set(ident.values())
    ball = {i: {i} for i in kept}
    seen = set()                                           # every E_s(j) of the layers below
    for r in range(1, radius + 1):
        ident = {i: mix(mix(ident[i], r), sum(mix(ident[j], w) for j, w in nbr[i].items()) & MASK) for i in kept}
        env = {i: frozenset(frozenset((a, c)) for a in ball[i] for c in nbr[a]) for i in kept}      # bonds with an end in ball_{r-1}(i)
        lowest = {}
        for i in kept:
            if env[i] and env[i] not in seen:
                lowest[env[i]] = min(lowest.get(env[i], ident[i]), ident[i])
        features |= set(lowest.values())
        seen |= set(env.values())
        ball = {i: ball[i] | {c for a in ball[i] for c in nbr[a]} for i in kept}
    return features


def fold(features, n_bits):
    return set(features) if not n_bits else {f % n_bits for f in features}


def similarity_counts(a, b, drop_h=True, radius=2, n_bits=2048):
    """(common, |A|, |B|) of the two folded sets (``n_bits`` 0: unfolded)."""
    fa, fb = fold(fingerprint(a, drop_h, radius), n_bits), fold(fingerprint(b, drop_h, radius), n_bits)
    return len(fa & fb), len(fa), len(fb)


def tanimoto(common, na, nb):
    return 1.0 if na == 0 and nb == 0 else common / (na + nb - common)


def cosine(common, na, nb):
    if na == 0 and nb == 0:
        return 1.0
    return 0.0 if na == 0 or nb == 0 else common / float(np.sqrt(float(na) * float(nb)))


# ------------------------------------------------------------------------------------------------------------------ the hand table

def _mol(types, edges, orders=None):
    return GM.molecule(types, edges, orders=orders)


def _kekule(first):
    return [2 if k % 2 == first else 1 for k in range(6)]


RING = GM._path(0, 1, 2, 3, 4, 5, 0)
MOLECULES = {
    "methane": _mol([1], []),
    "ethane": _mol([1, 1], [(0, 1)]),
    "propane": _mol([1, 1, 1], [(0, 1), (1, 2)]),
    "cyclopropane": _mol([1, 1, 1], [(0, 1), (1, 2), (0, 2)]),
    "Kekule benzene": _mol([1] * 6, RING, _kekule(0)),
    "ethanol": _mol([1, 1, 3], [(0, 1), (1, 2)]),
    "dimethyl ether": _mol([1, 3, 1], [(0, 1), (1, 2)]),
    "o-xylene": _mol([1] * 8, RING + [(0, 6), (1, 7)], _kekule(0) + [1, 1]),          # the two methyls sit on ring atoms 0 and 1
    "o-xylene, the other drawing": _mol([1] * 8, RING + [(0, 6), (1, 7)], _kekule(1) + [1, 1]),
}
# heavy atoms only: number of features at R = 0, 1, 2, 3
HAND_COUNTS = {
    "methane": (1, 1, 1, 1),
    "ethane": (1, 2, 2, 2),
    "propane": (2, 4, 4, 4),
    "cyclopropane": (1, 2, 3, 3),
    "Kekule benzene": (1, 2, 3, 4),
    "ethanol": (3, 6, 6, 6),
    "dimethyl ether": (2, 4, 4, 4),
}
# at R = 2, unfolded: (common, |A|, |B|)
HAND_PAIRS = [
    ("propane", "cyclopropane", (0, 4, 3)),
    ("ethane", "propane", (1, 2, 4)),
    ("ethanol", "dimethyl ether", (1, 6, 4)),
    ("o-xylene", "o-xylene, the other drawing", (5, 10, 10)),
]


def dense_record():
    """A malformed record: 29 atoms of one type, every bond byte 255 - and in the lower triangle and on the diagonal bytes that the
    definition never reads.  (rec [1, 1248] u8, n [1] i32, the molecule the definition sees)."""
    from tests import structure_mirror as SM
    mol = GM.molecule([1] * SM.W, [(i, j) for i in range(SM.W) for j in range(i + 1, SM.W)], orders=[255] * (SM.W * (SM.W - 1) // 2))
    rec, n = SM.records([mol])
    noisy = rec.copy()
    block = noisy[0, SM.BOND:SM.BOND_END].reshape(SM.W, SM.W)
    block[np.tril_indices(SM.W)] = (np.arange(SM.W * (SM.W + 1) // 2) * 37 % 251 + 1).astype(np.uint8)
    return noisy, n, mol
