"""CPU yardstick of ``dsv_valence_records`` and ``dsv_fragment_records`` in plain Python, written from the text of
include/diffspectra_valence.h and not from the kernel: bond orders from the record or from fp32 distances, the 2-D / 3-D stability tables, the
applied-charge rule, the restated RDKit valence check, components by union-find, the tie rule of the largest fragment, and the extractor
byte for byte.  It works on raw record bytes, so whatever the contract says is ignored can hold garbage.

Also here: the metric arithmetic of ``get_edm_metric_2d`` / ``get_edm_metric_3d`` over a list of records (``edm_metric``), and small molecule
builders for the tests.
"""
from __future__ import annotations

import numpy as np

from tests import graph_mirror as GM, structure_mirror as SM

W, RECORD_BYTES = SM.W, SM.RECORD_BYTES
POS, TYPE, FC, BOND, BOND_END = SM.POS, SM.TYPE, SM.FC, SM.BOND, SM.BOND_END
RECORD, DISTANCE = 0, 1
OK, UNUSABLE = 0, 3

# allowed_fc_bonds (header): element -> {charge: allowed valences}
STABLE_2D = [
    {0: (1,), 1: (0,), -1: (0,)},
    {0: (3, 4), 1: (3,), -1: (3,)},
    {0: (2, 3), 1: (2, 3, 4), -1: (2,)},
    {0: (2,), 1: (3,), -1: (1,)},
    {0: (1,), -1: (0,)},
]
STABLE_3D = (1, 4, 3, 2, 1)                                                   # allowed_bonds
APPLIED = {(2, 1), (2, -1), (1, 1), (3, -1), (1, -1)}                         # atom_fc_num: N+1, N-1, C+1, O-1, C-1
VMAX = {(0, 0): 1, (1, 0): 4, (1, 1): 3, (1, -1): 3, (2, 0): 3, (2, 1): 4, (2, -1): 2, (3, 0): 2, (3, -1): 1, (4, 0): 1}
# single / double / triple lengths in pm, 0 = no such bond (the tables the header refers to: those of ds_check_stability)
L1 = [[74, 109, 101, 96, 92], [109, 154, 147, 143, 135], [101, 147, 145, 140, 136], [96, 143, 140, 148, 142], [92, 135, 136, 142, 142]]
L2 = [[0, 0, 0, 0, 0], [0, 134, 129, 120, 0], [0, 129, 125, 121, 0], [0, 120, 121, 121, 0], [0, 0, 0, 0, 0]]
L3 = [[0, 0, 0, 0, 0], [0, 120, 116, 113, 0], [0, 116, 110, 0, 0], [0, 113, 0, 0, 0], [0, 0, 0, 0, 0]]
THRESHOLDS = sorted({L1[a][b] + 10 for a in range(5) for b in range(5)} | {L2[a][b] + 5 for a in range(5) for b in range(5) if L2[a][b]}
                    | {L3[a][b] + 3 for a in range(5) for b in range(5) if L3[a][b]})


def clamp_n(n):
    return int(min(max(int(n), 0), W))


def scaled_distances(pos):
    """[n, n] fp32: 100 |r_i - r_j|, every operation rounded on its own, in the header's order (numpy float32 arithmetic does not fuse)."""
    p = np.asarray(pos, np.float32)
    d = p[:, None, :] - p[None, :, :]
    sq = d * d
    return np.sqrt((sq[..., 0] + sq[..., 1]) + sq[..., 2]) * np.float32(100.0)


def order_from_distance(ta, tb, d):
    order = 0
    if d < np.float32(L1[ta][tb] + 10):
        order = 1
        if L2[ta][tb] != 0 and d < np.float32(L2[ta][tb] + 5):
            order = 2
            if L3[ta][tb] != 0 and d < np.float32(L3[ta][tb] + 3):
                order = 3
    return order


def applied_charge(t, c):
    return c if (t, c) in APPLIED else 0


def read(rec, n, bonds_from):
    """(n, types, raw charges, orders [n][n] symmetric, usable, scaled distances or None) of one record row."""
    rec = np.ascontiguousarray(np.asarray(rec, np.uint8))
    n = clamp_n(n)
    types = [int(v) for v in rec[TYPE:TYPE + n]]
    usable = n > 0 and all(t <= 4 for t in types)
    orders = [[0] * n for _ in range(n)]
    dist = None
    if bonds_from == RECORD:
        raw = [int(v) for v in rec[FC:FC + n].view(np.int8)]
        bond = rec[BOND:BOND_END].reshape(W, W)
        for i in range(n):
            for j in range(i + 1, n):
                orders[i][j] = orders[j][i] = int(bond[i, j])               # the upper triangle decides
                usable = usable and bond[i, j] <= 3
    else:
        raw = [0] * n
        pos = rec[POS:TYPE].view(np.float32).reshape(W, 3)
        dist = scaled_distances(pos[:n])
        assert dist.dtype == np.float32
        if usable:
            for i in range(n):
                for j in range(i + 1, n):
                    orders[i][j] = orders[j][i] = order_from_distance(types[i], types[j], dist[i, j])
    return n, types, raw, orders, usable, dist


def components(n, orders):
    """Union-find over bonds of order > 0: the components as ascending atom lists, in the order of their lowest atom."""
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for i in range(n):
        for j in range(i + 1, n):
            if orders[i][j] > 0:
                a, b = find(i), find(j)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    groups = {}
    for i in range(n):
        groups.setdefault(find(i), []).append(i)
    return [groups[k] for k in sorted(groups)]


def bits(atoms):
    return sum(1 << i for i in atoms)


def analyse(rec, n, bonds_from=RECORD):
    """One row of ``dsv_valence_records``: dict(valence [29], stable_mask, valid_mask, summary (4), largest_mask, status)."""
    n, types, raw, orders, usable, _ = read(rec, n, bonds_from)
    if not usable:
        return dict(valence=[0] * W, stable_mask=0, valid_mask=0, summary=(0, 0, 0, 0), largest_mask=0, status=UNUSABLE)
    val = [sum(row) for row in orders]
    stable, valid = [], []
    for i in range(n):
        t, c = types[i], raw[i]
        if bonds_from == RECORD:
            table = STABLE_2D[t]
            ok = val[i] in (table[c] if c in table else table[0])
        else:
            ok = val[i] == STABLE_3D[t]
        if ok:
            stable.append(i)
        if val[i] <= VMAX[t, applied_charge(t, c)]:
            valid.append(i)
    comps = components(n, orders)
    largest = max(comps, key=len)                                             # max keeps the first of equal size: the lowest first atom
    return dict(valence=val + [0] * (W - n), stable_mask=bits(stable), valid_mask=bits(valid),
                summary=(n, len(stable), len(comps), len(largest)), largest_mask=bits(largest), status=OK)


def flags(row):
    """(mol_stable, valid, complete) of one analysed row, as the ``Valence`` properties derive them."""
    n, n_stable, fragments, _ = row["summary"]
    usable = row["status"] == OK
    valid = usable and row["valid_mask"] == (1 << n) - 1
    return usable and n_stable == n, valid, valid and fragments == 1


def fragment(rec, n, keep, bonds_from=RECORD, charge_rule=True):
    """One row of ``dsv_fragment_records``: (record bytes uint8 [1248], out_n)."""
    n, types, raw, orders, usable, _ = read(rec, n, bonds_from)
    out = np.zeros(RECORD_BYTES, np.uint8)
    if not usable:
        return out, 0
    rec = np.ascontiguousarray(np.asarray(rec, np.uint8))
    atoms = [i for i in range(n) if (int(keep) >> i) & 1]
    m = len(atoms)
    pos_in = rec[POS:TYPE].reshape(W, 12)
    out_pos, out_bond = out[POS:TYPE].reshape(W, 12), out[BOND:BOND_END].reshape(W, W)
    for r, i in enumerate(atoms):
        out_pos[r] = pos_in[i]                                                # the fp32 bit patterns
        out[TYPE + r] = types[i]
        charge = applied_charge(types[i], raw[i]) if charge_rule else raw[i]
        out[FC + r] = np.array(charge, np.int8).view(np.uint8)
        for s, j in enumerate(atoms):
            out_bond[r, s] = orders[i][j]
    return out, m


def analyse_table(rec, n, bonds_from=RECORD):
    return [analyse(r, k, bonds_from) for r, k in zip(np.asarray(rec), np.asarray(n))]


def fragment_table(rec, n, keep, bonds_from=RECORD, charge_rule=True):
    rows = [fragment(r, k, m, bonds_from, charge_rule) for r, k, m in zip(np.asarray(rec), np.asarray(n), np.asarray(keep))]
    return np.stack([r for r, _ in rows]) if rows else np.zeros((0, RECORD_BYTES), np.uint8), np.array([m for _, m in rows], np.int32)


def edm_metric(rec, n, bonds_from=RECORD, known=None):
    """The six numbers of ``get_edm_metric_2d`` / ``_3d`` with the denominators of ``eval_rdmol``: ``known`` is a list of molecule dicts or None."""
    rec, n = np.asarray(rec), np.asarray(n)
    rows = analyse_table(rec, n, bonds_from)
    P, atoms = len(rows), sum(clamp_n(k) for k in n)
    f = [flags(r) for r in rows]
    largest = []
    for r, k, row, (_, valid, _) in zip(rec, n, rows, f):
        if valid:
            out, m = fragment(r, k, row["largest_mask"], bonds_from, True)
            largest.append(SM.mol_from_record(out, m))
    distinct = []
    for mol in largest:
        if not any(GM.same_graph(mol, other) for other in distinct):
            distinct.append(mol)
    novel = -1 if known is None else sum(1 for mol in distinct if not any(GM.same_graph(mol, k) for k in known)) / P
    return dict(mol_stable=sum(a for a, _, _ in f) / P, atom_stable=sum(r["summary"][1] for r in rows) / atoms, Validity=sum(b for _, b, _ in f) / P,
                Complete=sum(c for _, _, c in f) / P, Unique=len(distinct) / P, Novelty=novel)


# ------------------------------------------------------------------------------------------------------------------ molecules

def molecule(types, bonds, fc=None, pos=None):
    """Molecule dict from ``bonds = [(i, j, order)]``."""
    mol = GM.molecule(types, [(i, j) for i, j, _ in bonds], fc=fc, orders=[o for _, _, o in bonds])
    if pos is not None:
        mol["pos"] = np.asarray(pos, np.float64)
    return mol


def chain(n, rng=None, t=1):
    """A chain of n atoms of type t; with ``rng`` the atoms are numbered at random."""
    mol = molecule([t] * n, [(i, i + 1, 1) for i in range(n - 1)])
    return mol if rng is None else GM.permuted(mol, rng)


def ring(n, rng=None):
    mol = molecule([1] * n, [(i, (i + 1) % n, 1) for i in range(n)])
    return mol if rng is None else GM.permuted(mol, rng)


def near_threshold(scaled, margin=0.01):
    """True when a scaled distance (or any off-diagonal entry of a matrix of them) lies closer than ``margin`` to a threshold of the tables."""
    d = np.asarray(scaled, np.float64)
    if d.ndim == 2:
        d = d[~np.eye(d.shape[0], dtype=bool)]
    return bool((np.abs(d.reshape(-1, 1) - np.asarray(THRESHOLDS, np.float64)) < margin).any())
