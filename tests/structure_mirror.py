"""CPU yardstick of ``ds_match_records`` (include/diffspectra_hip.h): numpy float64 + ``scipy.optimize.linear_sum_assignment``.

The reference's ``eval_sampled_mols/rmsd.py`` needs RDKit and cannot run here, so this module RESTATES its steps on plain arrays, each with
the line of the reference it stands for (as ``oracle/`` does for the model); nothing of the reference's text is copied.  Two outputs
(``bond_acc``, ``exact``) are extensions of this project and are defined in the header.  A molecule is a dict ``pos [n,3] f64 (the fp32 values
of the record), type [n] (0..4 = H, C, N, O, F), fc [n], bond [n,n]`` - what ``mol_from_record`` reads out of a 1 248-byte record.

Also here: the seeded generator of synthetic (ground truth, candidate) pairs the GPU parity tests and the measurement share.
"""
from __future__ import annotations

import numpy as np
from scipy.optimize import linear_sum_assignment

W = 29                       # atoms per record (DS_MAX_ATOMS)
RECORD_BYTES = 1248
# byte offsets of a record's fields and the end of the bond block: plain numbers on purpose - this mirror is a yardstick of the header's
# DS_REC_* and of shard.pack_records_u8 (tests/test_record_pairs_cpu.py compares the three), so it does not import them
POS, TYPE, FC, BOND, BOND_END = 0, 348, 377, 406, 1247


def mol_from_record(rec, n):
    """Record row (uint8 [1248], layout of ``shard.pack_records_u8``) -> molecule dict of its first ``n`` atoms."""
    rec = np.ascontiguousarray(np.asarray(rec, dtype=np.uint8))
    n = int(min(max(int(n), 0), W))
    pos = rec[POS:TYPE].view(np.float32).reshape(W, 3)[:n].astype(np.float64)
    return dict(pos=pos, type=rec[TYPE:FC][:n].astype(np.int64), fc=rec[FC:BOND].view(np.int8)[:n].astype(np.int64),
                bond=rec[BOND:BOND_END].reshape(W, W)[:n, :n].astype(np.int64))


def records(mols):
    """(rec [len, 1248] u8, n [len] i32) of a list of molecule dicts, in the layout of ``shard.pack_records_u8`` (written here with numpy
    because thousands of molecules go through it; tests/test_graph_identity_cpu.py compares it with the project's packer)."""
    rec = np.zeros((len(mols), RECORD_BYTES), np.uint8)
    for k, m in enumerate(mols):
        n = len(m["type"])
        pos, bond = np.zeros((W, 3), np.float32), np.zeros((W, W), np.uint8)
        pos[:n], bond[:n, :n] = m["pos"], np.asarray(m["bond"]).astype(np.uint8)
        rec[k, POS:TYPE] = pos.reshape(-1).view(np.uint8)
        rec[k, TYPE:TYPE + n] = np.asarray(m["type"]).astype(np.uint8)
        rec[k, FC:FC + n] = np.asarray(m["fc"]).astype(np.int8).view(np.uint8)
        rec[k, BOND:BOND_END] = bond.reshape(-1)
    return rec, np.array([len(m["type"]) for m in mols], np.int32)


def record_from_mol(pos, atom_type, fc, bond):
    """The inverse, through the project's own packer (positions are rounded to fp32 there)."""
    import torch
    from diffspectra_amd.shard import pack_records_u8
    n = len(atom_type)
    t = lambda a, dt: torch.as_tensor(np.asarray(a), dtype=dt).reshape((1, n) + tuple(np.asarray(a).shape[1:]))
    return pack_records_u8(t(pos, torch.float32), t(atom_type, torch.int64), t(fc, torch.int64), t(bond, torch.int64))[0].numpy()


def bond_between(mol, i, j):
    """Bond order of an unordered atom pair: the upper triangle of the record's matrix (the packer writes a symmetric one)."""
    return int(mol["bond"][min(i, j), max(i, j)])


def largest_fragment(mol):
    """Original indices (ascending) of the largest connected fragment; a bond is an order > 0 (rmsd.py:82-86: ``GetMolFrags`` lists
    fragments by their lowest atom index and ``max`` keeps the first of equal size - RDKit behaviour restated, not executed here)."""
    n = len(mol["type"])
    seen, best = [False] * n, []
    for s in range(n):                                # fragments in the order of their lowest atom
        if seen[s]:
            continue
        comp, stack = [], [s]
        seen[s] = True
        while stack:
            a = stack.pop()
            comp.append(a)
            for b in range(n):
                if not seen[b] and b != a and bond_between(mol, a, b) > 0:
                    seen[b] = True
                    stack.append(b)
        if len(comp) > len(best):                     # strictly larger: the first of equal size stays
            best = comp
    return sorted(best)


def _penalty(ta, tb):
    """rmsd.py:190-198 on decoder indices (S never occurs in QM9): 0 same, 2 both in {C, N, O}, 10 otherwise."""
    same = ta[:, None] == tb[None, :]
    light = ((ta >= 1) & (ta <= 3))[:, None] & ((tb >= 1) & (tb <= 3))[None, :]
    return np.where(same, 0.0, np.where(light, 2.0, 10.0))


def _cost(xp, xr, tp, tr, jitter):
    """rmsd.py:176-188: rows generated atoms, columns ground-truth atoms, distance + penalty."""
    d = np.sqrt(((xp[:, None, :] - xr[None, :, :]) ** 2).sum(-1)) + _penalty(tp, tr)
    if jitter is not None:
        d = d + jitter.choice([-1e-7, 1e-7], size=d.shape)
    return d


def _match(cost, max_distance):
    """rmsd.py:153-174: clip entries above max_distance to 1000 (finite max_distance only), assign, keep matches within it.
    Returns ({generated: ground truth}, clipped cost matrix)."""
    c = cost
    if np.isfinite(max_distance):
        c = cost.copy()
        c[c > max_distance] = 1000.0
    rows, cols = linear_sum_assignment(c)
    lim = max_distance if np.isfinite(max_distance) else np.inf
    return {int(p): int(r) for p, r in zip(rows, cols) if c[p, r] <= lim}, c


def match_pair(prb, ref, max_distance=5.0, min_atoms=3, jitter=None, want_internals=False):
    """One pair -> dict(valid, rmsd, n_matched, type_acc, bond_acc, exact, map [29] of original indices).  rmsd.py:12-73.
    ``max_distance`` is compared as the fp32 value the C entry point receives.  ``jitter``: a ``numpy.random.Generator`` that perturbs every
    cost entry of both matches by +-1e-7 (the tie precondition of the parity test)."""
    max_distance = float(np.float32(max_distance))
    out = dict(valid=False, rmsd=float("nan"), n_matched=0, type_acc=np.float32(0), bond_acc=np.float32(0), exact=0,
               map=np.full(W, -1, dtype=np.int64))
    fp, fr = largest_fragment(prb), largest_fragment(ref)                             # rmsd.py:28-29
    if min(len(fp), len(fr)) < max(min_atoms, 1):     # the unclipped first match assigns min(np, nr) atoms; fewer than min_atoms can never become
        return out                                    # valid (rmsd.py:49-52 falls back to PCA, rmsd.py:64 then rejects the pair)
    xp, xr = prb["pos"][fp], ref["pos"][fr]
    if not (np.isfinite(xp).all() and np.isfinite(xr).all()):     # linear_sum_assignment raises on such a matrix: rmsd.py:164-168 -> no map
        return out
    xp, xr = xp - xp.mean(0, keepdims=True), xr - xr.mean(0, keepdims=True)           # rmsd.py:40-41,106-109
    tp, tr = prb["type"][fp], ref["type"][fr]
    tmp, _ = _match(_cost(xp, xr, tp, tr, jitter), np.inf)                            # rmsd.py:45-48
    keys = sorted(tmp)
    H = xp[keys].T @ xr[[tmp[k] for k in keys]]                                       # rmsd.py:55-57,117
    U, S, Vt = np.linalg.svd(H)
    R = U @ Vt
    if np.linalg.det(R) < 0:                                                          # rmsd.py:121-123
        Vt[-1, :] *= -1
        R = U @ Vt
    xa = xp @ R                                                                       # rmsd.py:58,126-128
    final, clipped = _match(_cost(xa, xr, tp, tr, jitter), max_distance)              # rmsd.py:61-63
    out["n_matched"] = len(final)
    if want_internals:
        out["internals"] = dict(xa=xa, xr=xr, tp=tp, tr=tr, fp=fp, fr=fr, clipped=clipped, sv=S)
    if len(final) < max(min_atoms, 1):                                                # rmsd.py:64-65
        return out
    ks = sorted(final)
    d2 = [float(((xa[k] - xr[final[k]]) ** 2).sum()) for k in ks]                      # rmsd.py:200-208
    n_type = sum(int(tp[k] == tr[final[k]]) for k in ks)                              # rmsd.py:211-227
    n_fc = sum(int(prb["fc"][fp[k]] == ref["fc"][fr[final[k]]]) for k in ks)
    pairs = [(a, b) for i, a in enumerate(ks) for b in ks[i + 1:]]
    n_bond = sum(int(bond_between(prb, fp[a], fp[b]) == bond_between(ref, fr[final[a]], fr[final[b]])) for a, b in pairs)
    whole = len(fp) == len(prb["type"]) and len(fr) == len(ref["type"]) and len(fp) == len(fr)
    out.update(valid=True, rmsd=float(np.sqrt(np.mean(d2))), type_acc=np.float32(n_type / len(ks)),
               bond_acc=np.float32(n_bond / len(pairs)) if pairs else np.float32(0),
               exact=int(whole and len(ks) == len(fp) and n_type == len(ks) and n_fc == len(ks) and n_bond == len(pairs)))
    for k in ks:
        out["map"][fp[k]] = fr[final[k]]
    return out


def second_match_score(internals, gmap):
    """Total clipped cost of the second assignment that a map over ORIGINAL indices stands for, on this mirror's aligned coordinates
    (atoms of the smaller side that the map leaves out cost 1000 each, as a clipped assignment charges them)."""
    fp, fr, c = internals["fp"], internals["fr"], internals["clipped"]
    kp, kr = {a: i for i, a in enumerate(fp)}, {a: i for i, a in enumerate(fr)}
    total, used = 0.0, 0
    for a, b in enumerate(gmap):
        if b >= 0:
            if a not in kp or int(b) not in kr:
                return float("inf")
            total += c[kp[a], kr[int(b)]]
            used += 1
    return total + 1000.0 * (min(len(fp), len(fr)) - used)


def match_batch(prb_rec, prb_n, ref_rec, ref_n, ref_index=None, max_distance=5.0, min_atoms=3, jitter=None, want_internals=False):
    """``match_pair`` over record arrays ``[P,1248]`` / ``[M,1248]`` -> list of result dicts."""
    res = []
    for p in range(len(prb_rec)):
        r = p if ref_index is None else int(ref_index[p])
        res.append(match_pair(mol_from_record(prb_rec[p], prb_n[p]), mol_from_record(ref_rec[r], ref_n[r]), max_distance, min_atoms,
                              jitter, want_internals))
    return res


# ------------------------------------------------------------------------------------------------------------------ synthetic pairs

QM9_TYPE_MIX = (0.51, 0.35, 0.06, 0.075, 0.005)       # H, C, N, O, F: roughly the QM9 atom census


def random_tree_molecule(rng, n):
    """A bonded tree of ``n`` atoms: every new atom hangs 1.0-1.6 A from a random earlier one, at least 0.9 A from all others."""
    pos = np.zeros((n, 3))
    bond = np.zeros((n, n), dtype=np.int64)
    k = 1
    while k < n:
        parent = int(rng.integers(k))
        v = rng.normal(size=3)
        cand = pos[parent] + v / np.linalg.norm(v) * rng.uniform(1.0, 1.6)
        if np.sqrt(((pos[:k] - cand) ** 2).sum(1)).min() < 0.9:
            continue
        pos[k] = cand
        bond[parent, k] = bond[k, parent] = int(rng.choice([1, 1, 1, 2, 3]))
        k += 1
    types = rng.choice(5, size=n, p=QM9_TYPE_MIX)
    fc = rng.choice([0, 0, 0, 0, 0, 0, 0, 0, 1, -1], size=n)
    return pos, types.astype(np.int64), fc.astype(np.int64), bond


def _rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def synthetic_pairs(count, seed, sizes=None):
    """(ref_rec [count,1248] u8, ref_n [count] i32, prb_rec, prb_n): seeded ground-truth trees of 3-29 atoms (or of ``sizes``) and one
    candidate each - the ground truth under a random proper rotation, a shift, a permutation and Gaussian noise of 0.02 / 0.1 / 0.3 / 0.6 A;
    a fifth of the pairs with ~20 % of the types substituted and one atom detached, another fifth with ~15 % of the atoms dropped and one
    atom moved 8 A away."""
    rng = np.random.default_rng(seed)
    ref_rec, prb_rec = np.zeros((count, RECORD_BYTES), np.uint8), np.zeros((count, RECORD_BYTES), np.uint8)
    ref_n, prb_n = np.zeros(count, np.int32), np.zeros(count, np.int32)
    for p in range(count):
        n = int(sizes[p]) if sizes is not None else int(rng.integers(3, W + 1))
        pos, types, fc, bond = random_tree_molecule(rng, n)
        ref_rec[p], ref_n[p] = record_from_mol(pos, types, fc, bond), n
        cpos = pos @ _rotation(rng) + rng.uniform(-3, 3, size=(1, 3)) + rng.normal(size=(n, 3)) * (0.02, 0.1, 0.3, 0.6)[p % 4]
        ctypes_, cfc, cbond = types.copy(), fc.copy(), bond.copy()
        kind = (p // 4) % 5
        if kind == 1:
            sub = rng.random(n) < 0.2
            ctypes_[sub] = rng.integers(0, 5, size=int(sub.sum()))
            a = int(rng.integers(n))
            cbond[a, :] = 0
            cbond[:, a] = 0
        elif kind == 2:
            keep = np.sort(rng.permutation(n)[:max(n - max(1, int(round(0.15 * n))), 1)])
            cpos, ctypes_, cfc, cbond = cpos[keep], ctypes_[keep], cfc[keep], cbond[np.ix_(keep, keep)]
            v = rng.normal(size=3)
            cpos[int(rng.integers(len(keep)))] += v / np.linalg.norm(v) * 8.0
        perm = rng.permutation(len(ctypes_))
        prb_rec[p] = record_from_mol(cpos[perm], ctypes_[perm], cfc[perm], cbond[np.ix_(perm, perm)])
        prb_n[p] = len(perm)
    return ref_rec, ref_n, prb_rec, prb_n
