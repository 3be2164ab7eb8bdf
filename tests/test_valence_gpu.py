"""GPU: ``dsv_valence_records`` and ``dsv_fragment_records`` (csrc/ds_valence.hip) against the plain-Python mirror of tests/valence_mirror.py,
which is written from include/diffspectra_valence.h and pinned to the reference's own results by tests/test_valence_cpu.py.  Every output is
an integer or a byte and is compared exactly; there is no tolerance anywhere.  The one condition is on INPUTS: where the bond orders come
from distances and the yardstick is the mirror (numpy fp32), the scaled distances stay 0.01 away from every threshold, and the test asserts
that; against ``ds_check_stability``, which shares the kernel's arithmetic, the inputs sit on the thresholds on purpose."""
import json
import os

import numpy as np
import pytest
import torch

from diffspectra_amd import engine as E, shard, structure_metrics as S
from tests import graph_mirror as GM, structure_mirror as SM, valence_mirror as VM
from tests.helpers import to_dev

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g19_stability2d.npz")
KEYS = ("valence", "stable_mask", "valid_mask", "summary", "largest_mask", "status")
FULL = (1 << 29) - 1


def on(dev, rec, n):
    return to_dev(dev, rec, torch.uint8), to_dev(dev, n, torch.int32)


def gpu_rows(dev, rec, n, mode=0):
    """``valence_records`` as the mirror's list of row dicts."""
    out = [t.cpu() for t in E.valence_records(*on(dev, rec, n), mode)]
    assert [t.dtype for t in out] == [torch.uint8, torch.int32, torch.int32, torch.int32, torch.int32, torch.uint8]
    assert [tuple(t.shape[1:]) for t in out] == [(29,), (), (), (4,), (), ()]
    val, stable, valid, summary, largest, status = (t.tolist() for t in out)
    return [dict(valence=val[p], stable_mask=stable[p], valid_mask=valid[p], summary=tuple(summary[p]), largest_mask=largest[p], status=status[p])
            for p in range(len(status))]


def gpu_fragments(dev, rec, n, keep, mode=0, charge_rule=True):
    out_rec, out_n = E.fragment_records(*on(dev, rec, n), to_dev(dev, keep, torch.int32), mode, charge_rule)
    assert out_rec.dtype == torch.uint8 and out_rec.shape == (len(n), E.RECORD_BYTES) and out_n.dtype == torch.int32
    return out_rec.cpu().numpy(), out_n.cpu().numpy()


def check_all_outputs(dev, rec, n, mode=0):
    """All ten output tensors against the mirror: the six of the analysis, the largest fragment under the charge rule, and the whole molecule
    with the raw charges.  Returns the mirror's rows."""
    want = VM.analyse_table(rec, n, mode)
    got = gpu_rows(dev, rec, n, mode)
    for p, (g, w) in enumerate(zip(got, want)):
        assert g == w, (p, int(n[p]), {k: (g[k], w[k]) for k in KEYS if g[k] != w[k]})
    largest = np.array([w["largest_mask"] for w in want], np.int32)
    for keep, rule in ((largest, True), (np.full(len(n), -1, np.int32), False)):
        g_rec, g_n = gpu_fragments(dev, rec, n, keep, mode, rule)
        w_rec, w_n = VM.fragment_table(rec, n, keep, mode, rule)
        assert np.array_equal(g_n, w_n)
        bad = np.nonzero((g_rec != w_rec).any(1))[0]
        assert bad.size == 0, (bad[:5], np.nonzero(g_rec[bad[0]] != w_rec[bad[0]])[0][:10])
    return want


def golden_molecules():
    rows = json.loads(str(np.load(GOLDEN)["molecules"]))
    return rows, [VM.molecule(r["types"], [tuple(b) for b in r["bonds"]], fc=r["charges"]) for r in rows]


def hand_molecules():
    H, Cc, N, O, F = range(5)
    rng = np.random.default_rng(7)
    return [
        VM.molecule([H, O, H, O, H, H, Cc], [(1, 4, 1), (1, 5, 1), (3, 0, 1), (3, 2, 1)]),
        VM.molecule([O, H, H, H], [(0, 1, 1), (0, 2, 1), (0, 3, 1)], fc=[1, 0, 0, 0]),
        VM.molecule([H, Cc, H, Cc, O, H, H, H, H], [(1, 3, 1), (3, 4, 1), (0, 1, 1), (2, 1, 1), (5, 1, 1), (6, 3, 1), (7, 3, 1), (8, 4, 1)],
                    fc=[1, 0, 0, 2, -1, 0, 0, 0, 0], pos=np.arange(27).reshape(9, 3)),
        VM.chain(29), VM.chain(29, rng), VM.ring(29, rng), GM.k29(), GM.nonane(), GM.permuted(GM.nonane(), rng), VM.molecule([F], [], fc=[-1]),
    ]


# ------------------------------------------------------------------------------------------------------------------ molecules

def test_golden_and_hand_molecules_against_the_mirror(gpu_device):
    rows, mols = golden_molecules()
    rec, n = SM.records(mols + hand_molecules())
    want = check_all_outputs(gpu_device, rec, n)
    # ... and so against the reference's recorded results
    for row, w in zip(rows, want):
        assert (w["summary"][0], w["summary"][1], VM.flags(w)[0]) == (row["ref_atom_num"], row["ref_nr_stable"], row["ref_stable"]), row["name"]
    full, m = gpu_fragments(gpu_device, rec[:len(rows)], n[:len(rows)], np.full(len(rows), FULL, np.int32))
    for row, r, k in zip(rows, full, m):
        assert SM.mol_from_record(r, k)["fc"].tolist() == row["ref_applied"], row["name"]


# ------------------------------------------------------------------------------------------------------------------ random records

def random_records(rng, P, garbage, mode=0, sizes=None):
    """(rec, n as given, clean rec): types 0..4, charges -2..+2, bond bytes 0..3 at densities 0.03 / 0.1 / 0.5, n from the sizes at which the
    kernel's paths change and two values that are clamped.  ``garbage``: random bytes in everything the contract says is ignored - atoms >= n,
    the lower triangle and the diagonal, the pad, and with mode 1 every bond and charge byte."""
    n = rng.choice([0, 1, 2, 3, 28, 29, -3, 40], size=P).astype(np.int32)
    if P >= 8:
        n[:8] = [0, 1, 2, 3, 28, 29, -3, 40]
    if sizes is not None:
        n[:] = sizes
    nc = np.clip(n, 0, 29)
    density = rng.choice([0.03, 0.1, 0.5], size=(P, 1, 1))
    bond = np.where(rng.random((P, 29, 29)) < density, rng.integers(1, 4, size=(P, 29, 29)), 0).astype(np.uint8)
    atom = np.arange(29)[None, :] < nc[:, None]                                               # [P, 29]
    pair = np.triu(np.ones((29, 29), bool), 1)[None] & atom[:, :, None] & atom[:, None, :]    # i < j < n
    rec = np.zeros((P, SM.RECORD_BYTES), np.uint8)
    pos = (rng.normal(size=(P, 29, 3)) * 1.2).astype(np.float32) * atom[:, :, None]
    rec[:, SM.POS:SM.TYPE] = pos.reshape(P, -1).view(np.uint8)
    rec[:, SM.TYPE:SM.FC] = rng.integers(0, 5, size=(P, 29)) * atom
    rec[:, SM.FC:SM.BOND] = (rng.integers(-2, 3, size=(P, 29)) * atom).astype(np.int8).view(np.uint8)
    rec[:, SM.BOND:SM.BOND_END] = (bond * pair).reshape(P, -1)
    if mode == 1:
        rec[:, SM.FC:SM.BOND_END] = 0
    clean = rec.copy()
    if garbage:
        ignored = np.zeros((P, SM.RECORD_BYTES), bool)
        ignored[:, SM.POS:SM.TYPE] = np.repeat(~atom, 12, axis=1)
        ignored[:, SM.TYPE:SM.FC] = ~atom
        ignored[:, SM.FC:SM.BOND] = ~atom
        ignored[:, SM.BOND:SM.BOND_END] = (~pair).reshape(P, -1)
        ignored[:, SM.BOND_END:] = True
        if mode == 1:
            ignored[:, SM.FC:SM.BOND_END] = True
        rec[ignored] = rng.integers(0, 256, size=int(ignored.sum()), dtype=np.uint8)
    return rec, n, clean


@pytest.mark.parametrize("P", [1, 63, 64, 65, 1000])
def test_random_records_against_the_mirror(gpu_device, P):
    rng = np.random.default_rng(20261201 + P)
    rec, n, clean = random_records(rng, P, garbage=True, sizes=[29] if P == 1 else None)
    want = check_all_outputs(gpu_device, rec, n)
    assert any(w["status"] == 3 for w in want) == bool((np.clip(n, 0, 29) == 0).any())
    if P >= 63:
        assert {w["summary"][0] for w in want} == {0, 1, 2, 3, 28, 29} and max(w["summary"][2] for w in want) > 3
        assert any(VM.flags(w)[1] for w in want) and any(not VM.flags(w)[1] for w in want if w["status"] == 0)
    # what the contract says is ignored is ignored: the same records with the garbage zeroed give the same bytes
    assert gpu_rows(gpu_device, clean, n) == gpu_rows(gpu_device, rec, n)
    keep = rng.integers(-2 ** 31, 2 ** 31, size=P).astype(np.int32)
    for rule in (True, False):
        a, b = gpu_fragments(gpu_device, rec, n, keep, 0, rule), gpu_fragments(gpu_device, clean, n, keep, 0, rule)
        w = VM.fragment_table(rec, n, keep, 0, rule)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[0], w[0]) and np.array_equal(a[1], w[1])


def test_chains_and_rings_of_29_atoms_under_random_renumbering(gpu_device):
    rng = np.random.default_rng(3)
    mols = [VM.chain(29)] + [VM.chain(29, rng) for _ in range(24)] + [VM.ring(29, rng) for _ in range(8)] + [VM.chain(k, rng) for k in range(1, 29)]
    mols.append(dict(VM.chain(29), bond=VM.chain(29)["bond"][::-1, ::-1].copy()))
    rec, n = SM.records(mols)
    got = gpu_rows(gpu_device, rec, n)
    for g, k in zip(got, n):
        assert g["summary"][2] == 1 and g["summary"][3] == k and g["largest_mask"] == (1 << int(k)) - 1 and g["status"] == 0
    assert got == VM.analyse_table(rec, n)
    # a 29-atom chain cut in two under random numberings: two fragments, the larger one wins wherever its atoms are
    cut = [GM.permuted(VM.molecule([1] * 29, [(i, i + 1, 1) for i in range(28) if i != c]), rng) for c in range(28)]
    rec, n = SM.records(cut)
    got = gpu_rows(gpu_device, rec, n)
    assert got == VM.analyse_table(rec, n)
    assert [g["summary"][2:] for g in got] == [(2, max(c + 1, 28 - c)) for c in range(28)]


def test_equal_fragments_tie_goes_to_the_lowest_atom(gpu_device):
    rng = np.random.default_rng(4)
    mols, first = [], []
    for k, size in ((2, 14), (3, 9), (4, 7), (7, 4), (9, 3), (14, 2), (29, 1), (2, 3)):
        for _ in range(4):
            perm = rng.permutation(k * size)
            groups = [sorted(int(a) for a in perm[g * size:(g + 1) * size]) for g in range(k)]
            bonds = [(g[i], g[i + 1], 1) for g in groups for i in range(size - 1)]
            mols.append(VM.molecule([1] * (k * size), bonds))
            first.append(VM.bits(min(groups)))                                  # the group holding atom 0
    rec, n = SM.records(mols)
    got = gpu_rows(gpu_device, rec, n)
    assert [g["largest_mask"] for g in got] == first and got == VM.analyse_table(rec, n)


def test_unusable_records(gpu_device):
    base, _ = SM.records([GM.nonane()] * 6)
    n = np.array([29, 29, 0, 29, 29, 20], np.int32)
    base[0, SM.TYPE + 28] = 5                                                   # a type byte above 4
    base[1, SM.BOND + 3 * 29 + 17] = 4                                          # a bond byte above 3, upper triangle
    base[3, SM.BOND + 17 * 29 + 3] = 4                                          # the same pair in the lower triangle: not looked at
    base[4, SM.BOND + 28 * 29 + 28] = 9                                         # the diagonal: not looked at
    base[5, SM.BOND + 20 * 29 + 25] = 4                                         # between atoms >= n: not looked at
    base[5, SM.TYPE + 20] = 77
    got = gpu_rows(gpu_device, base, n)
    zero = dict(valence=[0] * 29, stable_mask=0, valid_mask=0, summary=(0, 0, 0, 0), largest_mask=0, status=3)
    assert got[:3] == [zero] * 3 and [g["status"] for g in got[3:]] == [0, 0, 0] and got == VM.analyse_table(base, n)
    assert got[3] == got[4] and got[5]["summary"][0] == 20
    for mode in (0, 1):
        out, m = gpu_fragments(gpu_device, base, n, np.full(6, FULL, np.int32), mode)
        assert m[2] == 0 and not out[2].any() and m[0] == 0 and not out[0].any()
        assert (m[1] == 0 and not out[1].any()) == (mode == 0)                  # bond bytes do not exist for mode 1


# ------------------------------------------------------------------------------------------------------------------ orders from distances

class StabilityEngine:
    """What ``check_stability_batch`` needs of an engine, without weights."""

    def __init__(self, dev):
        self.device, self.lib = dev, E.load_library()

    def layout_for(self, node_mask):
        return E.Layout(node_mask, self.device), None

    check_stability = E.DmtEngine.check_stability


def near_threshold_molecules(rng, count):
    """Molecules of 2..29 atoms whose neighbours along a random walk sit within a few fp32 steps of a threshold of their element pair."""
    mols = []
    for k in range(count):
        n = int(rng.choice([2, 3, 5, 28, 29]))
        types = rng.integers(0, 5, size=n)
        pos = np.zeros((n, 3), np.float32)
        for i in range(1, n):
            a, b = int(types[i - 1]), int(types[i])
            ths = [VM.L1[a][b] + 10] + ([VM.L2[a][b] + 5] if VM.L2[a][b] else []) + ([VM.L3[a][b] + 3] if VM.L3[a][b] else [])
            d = np.float32(rng.choice(ths) / 100.0)
            d = np.nextafter(d, np.float32(rng.choice([0, 4])), dtype=np.float32) if rng.random() < 0.7 else d
            step = rng.normal(size=3)
            step[rng.integers(0, 3)] = 0.0 if rng.random() < 0.5 else step[0]
            pos[i] = pos[i - 1] + (step / np.linalg.norm(step) * d).astype(np.float32)
        mols.append(dict(pos=pos.astype(np.float64), type=types, fc=np.zeros(n, np.int64), bond=np.zeros((n, n), np.int64)))
    return mols


def test_distance_orders_equal_check_stability(gpu_device):
    """The same arithmetic as ``ds_check_stability``: equality on any input, so the inputs sit on the thresholds."""
    from diffspectra_amd.stability import check_stability_batch
    rng = np.random.default_rng(5)
    mols = near_threshold_molecules(rng, 150)
    for _ in range(50):
        n = int(rng.choice([1, 2, 9, 28, 29]))
        mols.append(dict(pos=(rng.normal(size=(n, 3)) * 1.3).astype(np.float32).astype(np.float64), type=rng.integers(0, 5, size=n),
                         fc=np.zeros(n, np.int64), bond=np.zeros((n, n), np.int64)))
    rec, n = SM.records(mols)
    B = len(mols)
    pos, types, mask = torch.zeros(B, 29, 3), torch.zeros(B, 29, dtype=torch.int64), torch.zeros(B, 29)
    for b, m in enumerate(mols):
        k = len(m["type"])
        pos[b, :k], types[b, :k], mask[b, :k] = torch.tensor(m["pos"], dtype=torch.float32), torch.tensor(m["type"]), 1
    d = gpu_device
    stable, nr, cnt, order = (t.cpu() for t in check_stability_batch(pos.to(d), types.to(d), mask.to(d), engine=StabilityEngine(d)))
    got = gpu_rows(d, rec, n, 1)
    out, m = gpu_fragments(d, rec, n, np.full(B, FULL, np.int32), 1)
    seen = set()
    for b in range(B):
        k = int(n[b])
        mine = out[b, SM.BOND:SM.BOND_END].reshape(29, 29)
        theirs = order[b, :k, :k].numpy() * (1 - np.eye(k, dtype=np.int64))       # ds_check_stability writes the pairs of atoms < n, not the diagonal
        assert m[b] == k and np.array_equal(mine[:k, :k], theirs) and not mine[k:].any() and not mine[:, k:].any(), b
        assert (got[b]["summary"][0], got[b]["summary"][1], VM.flags(got[b])[0]) == (int(cnt[b]), int(nr[b]), bool(stable[b])), b
        assert got[b]["valence"][:k] == theirs.sum(1).tolist()
        seen |= set(np.unique(mine).tolist())
    assert seen == {0, 1, 2, 3}
    # the walk did put pairs on the thresholds
    on_threshold = sum(VM.near_threshold(VM.scaled_distances(np.asarray(mm["pos"], np.float32)), 5e-3) for mm in mols[:150])
    assert on_threshold >= 140


def test_distance_orders_against_the_mirror(gpu_device):
    rng = np.random.default_rng(6)
    rec, n, clean = random_records(rng, 130, garbage=True, mode=1)
    # a condition on the INPUTS: 100 d stays at least 0.01 away from every threshold (numpy's fp32 and the GPU's agree anyway; this keeps the
    # test independent of that); a molecule that does not is drawn again
    for p in range(len(n)):
        k = int(np.clip(n[p], 0, 29))
        while VM.near_threshold(VM.scaled_distances(rec[p, SM.POS:SM.TYPE].view(np.float32).reshape(29, 3)[:k])):
            fresh = np.zeros((29, 3), np.float32)
            fresh[:k] = (rng.normal(size=(k, 3)) * 1.2).astype(np.float32)
            rec[p, :12 * k] = clean[p, :12 * k] = fresh.reshape(-1).view(np.uint8)[:12 * k]
    for p in range(len(n)):
        k = int(np.clip(n[p], 0, 29))
        assert not VM.near_threshold(VM.scaled_distances(rec[p, SM.POS:SM.TYPE].view(np.float32).reshape(29, 3)[:k]))
    want = check_all_outputs(gpu_device, rec, n, 1)
    assert {o for p in range(len(n)) for row in VM.read(rec[p], n[p], 1)[3] for o in row} == {0, 1, 2, 3}
    assert any(w["summary"][1] > 0 for w in want) and max(w["summary"][2] for w in want) > 1
    # bond and charge bytes are ignored in this mode
    assert gpu_rows(gpu_device, clean, n, 1) == gpu_rows(gpu_device, rec, n, 1)
    a, b = gpu_fragments(gpu_device, rec, n, np.full(len(n), FULL, np.int32), 1, False), gpu_fragments(gpu_device, clean, n, np.full(len(n), FULL, np.int32), 1, False)
    assert np.array_equal(a[0], b[0]) and not a[0][:, SM.FC:SM.BOND].any()


# ------------------------------------------------------------------------------------------------------------------ the extractor

def test_fragment_records_properties(gpu_device):
    rng = np.random.default_rng(8)
    mols = []
    for _ in range(120):                                                       # a connected molecule and a smaller one beside it: no tie to break
        b = int(rng.integers(1, 12))
        big, small = GM.random_molecule(rng, int(rng.integers(b + 1, 30 - b))), GM.random_molecule(rng, b)
        a = len(big["type"])
        bond = np.zeros((a + b, a + b), np.int64)
        bond[:a, :a], bond[a:, a:] = big["bond"], small["bond"]
        both = dict(pos=np.concatenate([big["pos"], small["pos"]]), type=np.concatenate([big["type"], small["type"]]),
                    fc=np.concatenate([big["fc"], small["fc"]]), bond=bond)
        mols.append(GM.permuted(both, rng))
    rec, n = SM.records(mols)
    want = VM.analyse_table(rec, n)
    largest = np.array([w["largest_mask"] for w in want], np.int32)
    out, m = gpu_fragments(gpu_device, rec, n, largest)
    # idempotent on its own output with a full mask
    again, m2 = gpu_fragments(gpu_device, out, m, np.full(len(m), -1, np.int32))
    assert np.array_equal(again, out) and np.array_equal(m2, m)
    # the graph hash of the largest fragment does not depend on the numbering of the input's atoms
    shuffled = [GM.permuted(mol, rng) for mol in mols]
    rec2, n2 = SM.records(shuffled)
    f2_rec, f2_n = S.largest_fragment_records(*on(gpu_device, rec2, n2))
    f1_rec, f1_n = S.largest_fragment_records(*on(gpu_device, rec, n))
    assert np.array_equal(f1_rec.cpu().numpy(), out) and torch.equal(f1_n, f2_n)
    assert torch.equal(E.graph_hash_records(f1_rec, f1_n), E.graph_hash_records(f2_rec, f2_n))
    # heavy atoms only, a mask of the caller's; charge rule on and off
    heavy = np.array([VM.bits(i for i, t in enumerate(mol["type"]) if t != 0) for mol in mols], np.int32)
    for rule in (True, False):
        g = gpu_fragments(gpu_device, rec, n, heavy, 0, rule)
        w = VM.fragment_table(rec, n, heavy, 0, rule)
        assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]) and not (g[0][:, SM.TYPE:SM.FC] == 0)[np.arange(29)[None] < g[1][:, None]].any()
    charged = VM.molecule([2, 3, 1, 0], [(0, 1, 1), (0, 2, 1), (0, 3, 1)], fc=[1, 1, 2, -1])
    rec, n = SM.records([charged])
    fc = lambda rule: SM.mol_from_record(*[x[0] for x in gpu_fragments(gpu_device, rec, n, np.array([15], np.int32), 0, rule)])["fc"].tolist()
    assert fc(True) == [1, 0, 0, 0] and fc(False) == [1, 1, 2, -1]


GUARD_ROWS = 3


def test_guarded_outputs_repeat_runs_and_batch_independence(gpu_device):
    """Every output between guard rows filled with a pattern (P = 65: a workgroup with three waves that have no record); two runs
    bit-identical; a row's outputs do not depend on the batch around it."""
    rng = np.random.default_rng(9)
    P = 65
    rec, n, _ = random_records(rng, P, garbage=True)
    rec_d, n_d = on(gpu_device, rec, n)
    lib, stream = E.load_library(), torch.cuda.current_stream().cuda_stream

    def guarded(width, dtype):
        raw = torch.full((P + 2 * GUARD_ROWS, width), 0x5A, dtype=torch.uint8, device=gpu_device).view(dtype)
        return raw, raw[GUARD_ROWS:GUARD_ROWS + P]

    def intact(raw):
        b = raw.view(torch.uint8)
        return bool((b[:GUARD_ROWS] == 0x5A).all()) and bool((b[-GUARD_ROWS:] == 0x5A).all())
    for mode in (0, 1):
        bufs = [guarded(29, torch.uint8), guarded(4, torch.int32), guarded(4, torch.int32), guarded(16, torch.int32), guarded(4, torch.int32), guarded(1, torch.uint8)]
        st = lib.dsv_valence_records(rec_d.data_ptr(), n_d.data_ptr(), P, mode, *(view.data_ptr() for _, view in bufs), stream)
        torch.cuda.synchronize()
        assert st == 0 and all(intact(raw) for raw, _ in bufs)
        plain = E.valence_records(rec_d, n_d, mode)
        again = E.valence_records(rec_d, n_d, mode)
        assert all(torch.equal(view.reshape(t.shape), t) and torch.equal(t, u) for (_, view), t, u in zip(bufs, plain, again))
        keep = to_dev(gpu_device, rng.integers(0, 2 ** 29, size=P), torch.int32)
        (r_raw, r_view), (n_raw, n_view) = guarded(E.RECORD_BYTES, torch.uint8), guarded(4, torch.int32)
        st = lib.dsv_fragment_records(rec_d.data_ptr(), n_d.data_ptr(), P, mode, keep.data_ptr(), 1, r_view.data_ptr(), n_view.data_ptr(), stream)
        torch.cuda.synchronize()
        assert st == 0 and intact(r_raw) and intact(n_raw)
        f_plain, f_again = E.fragment_records(rec_d, n_d, keep, mode), E.fragment_records(rec_d, n_d, keep, mode)
        assert torch.equal(r_view, f_plain[0]) and torch.equal(n_view.reshape(-1), f_plain[1]) and all(torch.equal(a, b) for a, b in zip(f_plain, f_again))
        # rows 5, 64 and 17 alone, and in another order
        for rows in ([64], [5], [17, 64, 5, 0]):
            idx = torch.tensor(rows, device=gpu_device)
            sub = E.valence_records(rec_d[idx].contiguous(), n_d[idx].contiguous(), mode)
            assert all(torch.equal(s, t[idx]) for s, t in zip(sub, plain))
            f_sub = E.fragment_records(rec_d[idx].contiguous(), n_d[idx].contiguous(), keep[idx].contiguous(), mode)
            assert all(torch.equal(s, t[idx]) for s, t in zip(f_sub, f_plain))


# ------------------------------------------------------------------------------------------------------------------ the metrics

NUMBERS = ("mol_stable", "atom_stable", "Validity", "Complete", "Unique", "Novelty")


def test_edm_metrics_against_the_mirror_and_the_reference_aggregation(gpu_device):
    z = np.load(GOLDEN)
    rows, mols = golden_molecules()
    dev = lambda ms: on(gpu_device, *SM.records(ms))
    for case in json.loads(str(z["eval_rdmol"])):
        known = None if case["known"] is None else [mols[k] for k in case["known"]]
        got = S.get_edm_metric_2d(known=None if known is None else dev(known))(*dev([mols[k] for k in case["rows"]]))
        assert {k: got[k] for k in case["result"]} == case["result"], case["name"]
    got = S.get_edm_metric_2d()(*dev(mols))
    assert got["mol_stable"] == sum(r["ref_stable"] for r in rows) / len(rows)
    assert got["atom_stable"] == sum(r["ref_nr_stable"] for r in rows) / sum(r["ref_atom_num"] for r in rows)
    assert got["valid"].dtype == torch.bool and got["valid"].device.type == "cuda" and isinstance(got["valence"], S.Valence)
    # alkanes and the golden molecules, repeats under other numberings, two molecules in one record, a few rows made unusable: the 2-D line
    # against the mirror-driven numbers; small random point sets (orders 0..3 from the distances): the 3-D line
    rng = np.random.default_rng(1)
    alkanes = [GM.saturated(GM.carbons(k, [(i, i + 1) for i in range(k - 1)])) for k in range(1, 9)]
    made = alkanes + mols + [GM.permuted(m, rng) for m in alkanes[:5] + mols[50:60]]
    rec2, n2 = SM.records(made)
    rec2[3, SM.TYPE] = 9
    n2[7] = 0
    rec3, n3, _ = random_records(rng, 120, garbage=True, mode=1, sizes=rng.choice([1, 2, 3, 4, 5], size=120))
    for fn, mode, rec, n, known in ((S.get_edm_metric_2d, VM.RECORD, rec2, n2, alkanes[::2] + mols[40:70:3]),
                                    (S.get_edm_metric_3d, VM.DISTANCE, rec3, n3, [SM.mol_from_record(*VM.fragment(rec3[p], n3[p], -1, 1)) for p in range(0, 120, 4)])):
        got = fn(known=dev(known))(*on(gpu_device, rec, n))
        want = VM.edm_metric(rec, n, mode, known)
        assert {k: got[k] for k in NUMBERS} == want, (mode, {k: got[k] for k in NUMBERS}, want)
        assert 0.0 < want["Novelty"] < want["Unique"] < want["Validity"] < 1.0 and 0.0 < want["Complete"] < want["Validity"]
        assert got["valid"].cpu().tolist() == [VM.flags(r)[1] for r in VM.analyse_table(rec, n, mode)]
        f_rec, f_n = S.largest_fragment_records(*on(gpu_device, rec, n), bonds="record" if mode == 0 else "distance")
        assert torch.equal(f_rec, got["largest"][0]) and torch.equal(f_n, got["largest"][1])
    v = S.valence_batch(*on(gpu_device, rec2, n2))
    assert not bool(v.usable[3]) and not bool(v.usable[7]) and bool(v.usable[0]) and v.complete.dtype == torch.bool and bool(v.mol_stable[0])


def test_evaluate_reports_the_edm_metrics(gpu_device, tmp_path, monkeypatch):
    """diffspectra_evaluate(structure_metrics=True) on filler weights, 3 steps: with ``cfg.eval.edm_metrics`` the 'structure' dict holds both
    lines, equal to a direct call on ``records_by_slot``; without the flag it has no new key; ``set_similarity`` is untouched by the flag."""
    from diffspectra_amd import filler, evaluate as EV
    from diffspectra_amd.config import qm9s_config
    from diffspectra_amd.dataset_pack import PackedSpectraTable
    from diffspectra_amd.registry import create_model
    import diffspectra_amd.dmt  # noqa: F401
    from tests.test_set_similarity_gpu import _graph_dataset
    cfg = qm9s_config("ir", device=gpu_device, steps=3, batch_size=4, num_samples=6)
    cfg.eval.begin_ckpt, cfg.eval.end_ckpt, cfg.eval.ckpts = 40, 40, ""
    table = PackedSpectraTable.from_dataset(_graph_dataset(8, seed=21), "ir", device=gpu_device)
    donor = create_model(cfg)
    donor.eval()
    filler.fill_module_(donor)
    ema = EV.ExponentialMovingAverage(donor.parameters(), decay=0.999)
    (tmp_path / "checkpoints").mkdir()
    EV.save_checkpoint(str(tmp_path / "checkpoints" / "checkpoint_40.pth"), dict(optimizer=None, model=donor, ema=ema, step=7))
    gather, kept = shard.gather_by_slot, []

    def gather_and_keep(rec, n_atoms):
        kept.append(gather(rec, n_atoms))
        return kept[-1]
    monkeypatch.setattr(shard, "gather_by_slot", gather_and_keep)
    cfg.eval.set_similarity = True
    torch.manual_seed(42)
    plain = EV.diffspectra_evaluate(cfg, str(tmp_path), table, structure_metrics=True)[40]["metrics"]["structure"]
    assert "metric_2d" not in plain and "metric_3d" not in plain
    cfg.eval.edm_metrics = True
    known = (table.gt_records[:3].clone(), table.num_atom[:3].clone())
    torch.manual_seed(42)
    res = EV.diffspectra_evaluate(cfg, str(tmp_path), table, structure_metrics=True, known_records=known)[40]
    monkeypatch.setattr(shard, "gather_by_slot", gather)
    st = res["metrics"]["structure"]
    assert set(st) == set(plain) | {"metric_2d", "metric_3d"}
    assert st["set_similarity"]["n_generated"] == plain["set_similarity"]["n_generated"] and st["set_similarity"]["snn"] == plain["set_similarity"]["snn"]
    n_atoms = torch.tensor([len(atom) for _, atom, _, _ in res["processed_mols"]])
    dev_known = (known[0].to(gpu_device), known[1])
    for key, fn in (("metric_2d", S.get_edm_metric_2d), ("metric_3d", S.get_edm_metric_3d)):
        direct = fn(known=dev_known)(kept[-1], n_atoms)
        assert set(st[key]) == set(NUMBERS) | {"valence", "valid", "largest"}
        assert {k: st[key][k] for k in NUMBERS} == {k: direct[k] for k in NUMBERS}
        assert all(0.0 <= st[key][k] <= 1.0 for k in NUMBERS)
        assert torch.equal(st[key]["valid"], direct["valid"]) and all(torch.equal(a, b) for a, b in zip(st[key]["valence"], direct["valence"]))
        assert st[key]["valid"].shape == (6,) and st[key]["valid"].device.type == "cuda"
