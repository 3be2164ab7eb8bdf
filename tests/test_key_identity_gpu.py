"""GPU: ``dsi_key_sites`` and ``dsi_key_identity_records`` (csrc/ds_key.hip) and what ``structure_metrics`` and ``evaluate`` build on them
against the plain-Python mirror of tests/key_mirror.py, which is written from include/diffspectra_key.h and pinned to hand-stated
expectations by tests/test_key_identity_cpu.py.  Flags, partners, masks, nodes, statuses, verdicts, counts and sites are compared exactly,
every returned map is checked here to be a normal-form isomorphism of the kind its verdict claims, the volumes agree within 1e-12."""
import collections

import numpy as np
import pytest
import torch

from diffspectra_amd import engine as E, shard, structure_metrics as S
from tests import graph_mirror as GM, key_mirror as K, stereo_mirror as ST, structure_mirror as SM
from tests.helpers import to_dev

pytestmark = pytest.mark.gpu

GUARD_ROWS = 3
W = K.W


def on(dev, mols):
    rec, n = SM.records(mols)
    return to_dev(dev, rec, torch.uint8), to_dev(dev, n, torch.int32)


@pytest.fixture(scope="module")
def table():
    """Every pair the comparisons run on, computed once, shared, never changed: the hand pairs, the pairs of the stereo table, the law-2 set,
    the shifted forms (and every third one reflected) against their molecule, and the first seed of stereo_mirror.seeded_pairs (n = 1 .. 12
    and one n = 29, whatever their valences) - a few hundred pairs - with the mirror's perception of every molecule and its answer."""
    mols = K.hand_molecules()
    prb = [mols[a] for a, _, _, _ in K.hand_pairs()] + [a for _, a, _, _ in K.stereo_table_pairs()]
    ref = [mols[b] for _, b, _, _ in K.hand_pairs()] + [b for _, _, b, _ in K.stereo_table_pairs()]
    hand = len(prb)
    a, b, _ = K.law2_pairs()
    prb, ref = prb + list(a), ref + list(b)
    for i, (_, _, m, s) in enumerate(K.shifted_forms()):
        prb, ref = prb + [s] + ([K.reflected(s)] if i % 3 == 0 else []), ref + [m] + ([m] if i % 3 == 0 else [])
    a, b, _ = ST.seeded_pairs(ST.SEEDS[:1])
    prb, ref = prb + list(a), ref + list(b)
    seen = {}

    def percept(m):
        if id(m) not in seen:
            seen[id(m)] = K.Perception(m)
        return seen[id(m)]
    pa, pb = [percept(m) for m in prb], [percept(m) for m in ref]
    want = [K.compare(x, y, pa=p, pb=q) for x, y, p, q in zip(prb, ref, pa, pb)]
    return dict(prb=prb, ref=ref, pa=pa, pb=pb, want=want, hand=hand)


def site_tensors(dev, mols, max_nodes=None, **kw):
    rec, n = on(dev, mols)
    out = E.key_sites(rec, n, max_nodes, **kw)
    assert [t.dtype for t in out] == [torch.uint8, torch.int32, torch.float64, torch.int32, torch.uint8]
    assert [tuple(t.shape) for t in out] == [(len(mols), W, 2), (len(mols), 9), (len(mols), W), (len(mols),), (len(mols),)]
    return out


def against_the_mirror(out, mols, percepts=None, max_nodes=K.DEFAULT_NODES):
    """Flags, partners, masks, nodes and status exactly; returns the largest |V - mirror| over the centres."""
    site, masks, volume, nodes, status = (t.cpu().numpy() for t in out)
    worst = 0.0
    for p, mol in enumerate(mols):
        row = K.site_rows(mol, max_nodes, found=None if percepts is None else percepts[p])
        assert status[p] == row["status"], p
        assert site[p].tolist() == row["site"].tolist(), (p, site[p].tolist(), row["site"].tolist())
        assert masks[p].tolist() == row["masks"], (p, masks[p].tolist(), row["masks"])
        assert nodes[p] == row["nodes"], p
        centres = row["site"][:, 0] & 3 == K.KIND_CENTRE
        assert not volume[p][~centres].any()
        both_nan = np.isnan(volume[p]) & np.isnan(row["volume"])
        diff = np.abs(np.where(both_nan, 0.0, volume[p] - row["volume"]))
        assert not np.isnan(diff).any()
        worst = max(worst, float(diff.max()))
    return worst


# ------------------------------------------------------------------------------------------------------------------ the sites

def test_sites_against_the_mirror(gpu_device, table):
    mols, percepts, seen = [], [], set()
    for m, p in zip(table["prb"] + table["ref"], table["pa"] + table["pb"]):
        if id(m) not in seen:
            seen.add(id(m))
            mols.append(m), percepts.append(p)
    assert 300 <= len(mols) <= 900
    out = site_tensors(gpu_device, mols)
    worst = against_the_mirror(out, mols, percepts)
    masks, status = out[1].cpu().numpy(), out[4].cpu().numpy()
    print(f"[key] sites of {len(mols)} records: {int((masks[:, 0] != 0).sum())} with centres, {int((masks[:, 3] != 0).sum())} with E/Z bonds, "
          f"{int((masks[:, 7] != 0).sum())} with a double bond on a shift path, {int((masks[:, 8] != 0).sum())} with a ring double bond, "
          f"max |V - mirror| {worst:.3e}")
    assert worst <= 1e-12
    assert not status.any()
    assert int((masks[:, 0] != 0).sum()) >= 40 and int((masks[:, 3] != 0).sum()) >= 20 and int((masks[:, 7] != 0).sum()) >= 40 and int((masks[:, 8] != 0).sum()) >= 20
    flags = out[0].cpu().numpy()[:, :, 0]
    assert int(((flags & K.HSLOT != 0) & (flags & 3 != 0)).any(1).sum()) >= 20, "sites that stand on a hydrogen slot"
    # row p lines up with row p of the normal form
    rec, n = on(gpu_device, mols)
    forms = E.normal_records(rec, n)
    out_n = forms[1].cpu().numpy()
    site = out[0].cpu().numpy()
    for p in range(len(mols)):
        assert not site[p, out_n[p]:, 0].any() and (site[p, out_n[p]:, 1] == K.NO_PARTNER).all()
        ends = np.nonzero(site[p, :, 0] & 3 == K.KIND_END)[0]
        assert all(site[p, site[p, e, 1], 1] == e for e in ends)


def test_sites_shape_edges_budget_and_thresholds(gpu_device):
    rng = np.random.default_rng(20261103)
    amide = lambda k: GM.molecule([1] * (k - 2) + [3, 2], [(i, i + 1) for i in range(k - 3)] + [(k - 3, k - 2), (k - 3, k - 1)], orders=[1] * (k - 3) + [2, 1])
    charged = amide(28)
    charged["fc"], charged["type"] = charged["fc"].copy(), charged["type"].copy()
    charged["type"][0], charged["fc"][0] = 2, 1
    loud = ST.fluoroethanol()
    loud["type"] = loud["type"].copy()
    loud["type"][2] = 7
    heavy = ST.fluoroethanol()
    heavy["bond"] = heavy["bond"].copy()
    heavy["bond"][0, 1] = heavy["bond"][1, 0] = 4
    lone = GM.molecule([1], [])
    hard = [GM.molecule([], []), lone, amide(29), amide(28), charged, GM.nonane(), GM.k29(), loud, heavy] + [GM.random_molecule(rng, 29) for _ in range(8)]
    for m in hard:
        m["pos"] = ST._f32(rng.normal(size=(len(m["type"]), 3)) * 1.5)
    out = site_tensors(gpu_device, hard)
    against_the_mirror(out, hard)
    status = out[4].cpu().tolist()
    assert status[:9] == [K.UNUSABLE, K.OK, K.OVERFLOW, K.OK, K.OVERFLOW, K.OK, K.OK, K.UNUSABLE, K.UNUSABLE]   # n = 0, n = 1, 30 nodes, exactly 29, 28 + group + proton
    for p in (0, 2, 4, 7, 8):                                                    # the defined row
        assert not out[0][p, :, 0].any() and (out[0][p, :, 1] == K.NO_PARTNER).all() and not out[1][p].any() and not out[2][p].any() and out[3][p] == 0
    # the budget: one node short is undecided with the defined row
    mols = K.hand_molecules()
    names = ["2-pyridone", "2-hydroxypyridine, N-C(OH)", "fumaric acid", "lactic acid", "(E)-3-hydroxyacrolein"]
    need = [K.Perception(mols[name]).nodes for name in names]
    assert min(need) >= 1
    for name, k in zip(names, need):
        exact, short = site_tensors(gpu_device, [mols[name]], k), site_tensors(gpu_device, [mols[name]], max(k - 1, 1))
        against_the_mirror(exact, [mols[name]], max_nodes=k)
        assert exact[4].item() == K.OK and exact[3].item() == k
        if k > 1:
            against_the_mirror(short, [mols[name]], max_nodes=k - 1)
            assert short[4].item() == K.ROW_UNDECIDED and short[3].item() == 0 and not short[0][0, :, 0].any() and not short[1].any()
    against_the_mirror(site_tensors(gpu_device, [mols[name] for name in names], E.MOBILE_MAX_NODES), [mols[name] for name in names], max_nodes=E.MOBILE_MAX_NODES)
    # other thresholds
    some = [mols["lactic acid"], mols["flattened 1-fluoroethanol"], mols["(E)-crotonic acid"]]
    for mv, mp in ((0.0, 0.0), (3.0, 0.99), (3.2, 1.1)):
        out = site_tensors(gpu_device, some, min_volume=mv, min_planarity=mp)
        site = out[0].cpu().numpy()
        for p, m in enumerate(some):
            assert site[p].tolist() == K.site_rows(m, min_volume=mv, min_planarity=mp)["site"].tolist()


# ------------------------------------------------------------------------------------------------------------------ the pairs

def key_pairs(dev, prb, ref, ref_index=None, max_nodes=4096, exhaustive=False):
    """``dsi_key_identity_records`` on the normal forms and site rows of both sides."""
    (p_rec, p_n), (r_rec, r_n) = on(dev, prb), on(dev, ref)
    p_form, r_form = E.normal_records(p_rec, p_n), E.normal_records(r_rec, r_n)
    p_site, r_site = E.key_sites(p_rec, p_n)[0], E.key_sites(r_rec, r_n)[0]
    out = E.key_identity_records(p_form[0], p_form[1], p_site, r_form[0], r_form[1], r_site, ref_index, max_nodes, exhaustive)
    assert [t.dtype for t in out] == [torch.uint8, torch.int32, torch.int32, torch.int32, torch.int32]
    return [t.cpu().numpy() for t in out]


@pytest.mark.parametrize("exhaustive", [False, True])
def test_identity_against_the_mirror(gpu_device, table, exhaustive):
    prb, ref, want = table["prb"], table["ref"], table["want"]
    assert 300 <= len(prb) <= 700
    verdict, nodes, found, sites, image = key_pairs(gpu_device, prb, ref, exhaustive=exhaustive)
    hist = collections.Counter()
    for k, w in enumerate(want):
        assert w["status"] == (K.OK, K.OK), "every record of the table has a normal form"
        assert verdict[k] == w["verdict"], (k, verdict[k], w["verdict"])
        assert sites[k].tolist() == w["sites"], k
        hist[int(verdict[k])] += 1
        if exhaustive:
            assert found[k].tolist() == w["found"], (k, found[k].tolist(), w["found"])
        else:                                                # stopped at the first same phi, or at the first isomorphism of an unassigned pair
            assert found[k][0] <= w["found"][0] and found[k][1] == min(w["found"][1], 1) and found[k][2] <= w["found"][2]
            if w["verdict"] in (K.MIRROR, K.STEREOISOMER, K.DIFFERENT):
                assert found[k].tolist() == w["found"], k
        assert K.map_claim(prb[k], ref[k], image[k], int(verdict[k]), table["pa"][k], table["pb"][k]), k
    assert set(hist) == {K.DIFFERENT, K.IDENTICAL, K.MIRROR, K.STEREOISOMER, K.UNASSIGNED} and min(hist.values()) >= 5, hist
    assert int(nodes.max()) >= 1 and int(found[:, 0].max()) >= 8
    hand = table["hand"]
    pairs = K.hand_pairs()
    assert verdict[:len(pairs)].tolist() == [v for _, _, v, _ in pairs], "the hand-stated table holds for the kernel"
    assert len(pairs) < hand


def test_pair_shape_edges_budget_reproducibility_and_guard_rows(gpu_device, table):
    """P = 67 pairs between guard rows filled with a pattern; ref_index inside and outside [0, M); empty records; a budget one node short;
    two runs bit-identical; one batch against the same batch split in two."""
    dev = gpu_device
    rng = np.random.default_rng(20261104)
    rows = rng.permutation(len(table["prb"]))[:64]
    prb = [table["prb"][r] for r in rows] + [GM.molecule([], []), GM.molecule([1], []), table["prb"][0]]
    ref = [table["ref"][r] for r in rows] + [GM.molecule([], []), GM.molecule([1], []), table["ref"][0]]
    for m in prb[64:66] + ref[64:66]:
        m["pos"] = np.zeros((len(m["type"]), 3))
    P = len(prb)
    (p_rec, p_n), (r_rec, r_n) = on(dev, prb), on(dev, ref)
    p_form, r_form = E.normal_records(p_rec, p_n), E.normal_records(r_rec, r_n)
    p_site, r_site = E.key_sites(p_rec, p_n)[0], E.key_sites(r_rec, r_n)[0]
    index = torch.arange(P, device=dev)
    index[3], index[9], index[P - 1] = -1, P, 0
    lib, stream = E.load_library(), torch.cuda.current_stream().cuda_stream

    def guarded(count, width, dtype):
        raw = torch.full((count + 2 * GUARD_ROWS, width), 0x5A, dtype=torch.uint8, device=dev).view(dtype)
        return raw, raw[GUARD_ROWS:GUARD_ROWS + count]

    def intact(raw):
        b = raw.view(torch.uint8)
        return bool((b[:GUARD_ROWS] == 0x5A).all()) and bool((b[-GUARD_ROWS:] == 0x5A).all())
    for exhaustive in (0, 1):
        bufs = [guarded(P, 1, torch.uint8), guarded(P, 4, torch.int32), guarded(P, 12, torch.int32), guarded(P, 16, torch.int32), guarded(P, 4 * W, torch.int32)]
        st = lib.dsi_key_identity_records(p_form[0].data_ptr(), p_form[1].data_ptr(), P, r_form[0].data_ptr(), r_form[1].data_ptr(), P, index.data_ptr(),
                                          p_site.data_ptr(), r_site.data_ptr(), 4096, exhaustive, *(view.data_ptr() for _, view in bufs), stream)
        torch.cuda.synchronize()
        assert st == 0 and all(intact(raw) for raw, _ in bufs)
        plain = E.key_identity_records(p_form[0], p_form[1], p_site, r_form[0], r_form[1], r_site, index, 4096, bool(exhaustive))
        again = E.key_identity_records(p_form[0], p_form[1], p_site, r_form[0], r_form[1], r_site, index, 4096, bool(exhaustive))
        assert all(torch.equal(view.reshape(t.shape), t) and torch.equal(t, u) for (_, view), t, u in zip(bufs, plain, again))
        verdict = plain[0].cpu().tolist()
        assert verdict[3] == verdict[9] == K.INVALID and not plain[1][[3, 9]].any() and not plain[2][[3, 9]].any() and not plain[3][[3, 9]].any() and (plain[4][[3, 9]] == -1).all()
        assert verdict[64] == K.DIFFERENT or verdict[64] == K.IDENTICAL          # two empty rows: whatever the graph kernels say of n = 0 ...
        assert verdict[64] == E.graph_identity_records(p_form[0][64:65], p_form[1][64:65], r_form[0][64:65], r_form[1][64:65])[0].item()
        assert verdict[65] == K.IDENTICAL and plain[4][65, 0] == 0               # ... and one atom is itself
        assert verdict[P - 1] == K.compare(prb[P - 1], ref[0])["verdict"]
        for k in range(64):
            if k not in (3, 9):
                assert verdict[k] == table["want"][rows[k]]["verdict"]
        # the same batch split in two, and single rows
        cut = 29
        parts = [E.key_identity_records(p_form[0][s].contiguous(), p_form[1][s].contiguous(), p_site[s].contiguous(), r_form[0], r_form[1], r_site,
                                        index[s].contiguous(), 4096, bool(exhaustive)) for s in (slice(0, cut), slice(cut, P))]
        assert all(torch.equal(torch.cat([a, b]), t) for a, b, t in zip(*parts, plain))
    # the budget: a pair one node short in the pair search is undecided whatever was found
    full = E.key_identity_records(p_form[0], p_form[1], p_site, r_form[0], r_form[1], r_site, None, 4096, True)
    used = full[1].cpu().numpy()
    k = int(np.argmax(used))
    assert used[k] >= 2 and full[2][k, 0] >= 1
    one = lambda budget: E.key_identity_records(p_form[0][k:k + 1], p_form[1][k:k + 1], p_site[k:k + 1], r_form[0][k:k + 1], r_form[1][k:k + 1], r_site[k:k + 1],
                                                None, budget, True)
    exact, short = one(int(used[k])), one(int(used[k]) - 1)
    assert exact[0].item() == full[0][k].item() and exact[1].item() == used[k]
    assert short[0].item() == K.UNDECIDED and short[1].item() == used[k] - 1 and (short[4] == -1).all() and short[2][0, 0] >= 1
    none = one(0)
    assert none[0].item() in (K.UNDECIDED, full[0][k].item()) and none[1].item() == 0
    # no pairs; the bindings refuse what the library would
    empty = E.key_identity_records(p_form[0][:0], p_form[1][:0], p_site[:0], r_form[0], r_form[1], r_site, None, 4096, False)
    assert [t.shape[0] for t in empty] == [0] * 5
    with pytest.raises(ValueError):
        E.key_identity_records(p_form[0], p_form[1], p_site[:5], r_form[0], r_form[1], r_site)
    with pytest.raises(TypeError):
        E.key_identity_records(p_form[0], p_form[1], p_site, r_form[0], r_form[1], r_site, None, 4096, 2)
    with pytest.raises(ValueError):
        E.key_sites(p_rec, p_n, 0)
    args = [view.data_ptr() for _, view in bufs]
    call = lambda nodes, exhaustive, site: lib.dsi_key_identity_records(p_form[0].data_ptr(), p_form[1].data_ptr(), P, r_form[0].data_ptr(), r_form[1].data_ptr(), P,
                                                                       index.data_ptr(), site, r_site.data_ptr(), nodes, exhaustive, *args, stream)
    assert call(-1, 0, p_site.data_ptr()) == -1 and call(4096, 2, p_site.data_ptr()) == -1 and call(4096, 0, 0) == -1
    torch.cuda.synchronize()
    assert all(intact(raw) for raw, _ in bufs)


def test_sites_guard_rows_repeats_and_batch_independence(gpu_device, table):
    """P = 65 records (a workgroup with three waves that have no record) between guard rows; two runs bit-identical; rows do not depend on
    the batch around them."""
    dev = gpu_device
    rng = np.random.default_rng(20261105)
    rows = rng.permutation(len(table["prb"]))[:65]
    mols = [table["prb"][r] for r in rows]
    rec, n = on(dev, mols)
    P = len(mols)
    lib, stream = E.load_library(), torch.cuda.current_stream().cuda_stream

    def guarded(count, width, dtype):
        raw = torch.full((count + 2 * GUARD_ROWS, width), 0x5A, dtype=torch.uint8, device=dev).view(dtype)
        return raw, raw[GUARD_ROWS:GUARD_ROWS + count]
    intact = lambda raw: bool((raw.view(torch.uint8)[:GUARD_ROWS] == 0x5A).all()) and bool((raw.view(torch.uint8)[-GUARD_ROWS:] == 0x5A).all())
    for budget in (K.DEFAULT_NODES, 1):
        bufs = [guarded(P, 2 * W, torch.uint8), guarded(P, 36, torch.int32), guarded(P, 8 * W, torch.float64), guarded(P, 4, torch.int32), guarded(P, 1, torch.uint8)]
        st = lib.dsi_key_sites(rec.data_ptr(), n.data_ptr(), P, budget, 0.5, 0.5, *(view.data_ptr() for _, view in bufs), stream)
        torch.cuda.synchronize()
        assert st == 0 and all(intact(raw) for raw, _ in bufs)
        plain, again = E.key_sites(rec, n, budget), E.key_sites(rec, n, budget)
        assert all(torch.equal(view.reshape(t.shape), t) and torch.equal(t, u) for (_, view), t, u in zip(bufs, plain, again))
        for sub in ([64], [5], [17, 64, 5, 0]):
            idx = torch.tensor(sub, device=dev)
            alone = E.key_sites(rec[idx].contiguous(), n[idx].contiguous(), budget)
            assert all(torch.equal(s, t[idx]) for s, t in zip(alone, plain))
    assert int((plain[4] == K.ROW_UNDECIDED).sum()) >= 3
    assert [t.shape[0] for t in E.key_sites(rec[:0], n[:0])] == [0] * 5


# ------------------------------------------------------------------------------------------------------------------ the public interface

def test_key_identity_batch_composition_and_the_laws(gpu_device, table):
    prb, ref, want = table["prb"], table["ref"], table["want"]
    prb_d, ref_d = on(gpu_device, prb), on(gpu_device, ref)
    got = S.key_identity_batch(ref_d, prb_d)
    assert isinstance(got, S.KeyIdentity)
    assert [t.dtype for t in got] == [torch.uint8, torch.int32, torch.int32, torch.int32, torch.int32, torch.uint8, torch.int8, torch.uint8, torch.uint8]
    verdict, strict, layer = got.verdict.cpu().tolist(), got.strict.cpu().tolist(), got.layer.cpu().tolist()
    stated = [K.identity(a, b) for a, b in zip(prb, ref)]
    assert verdict == [s[0] for s in stated] and strict == [s[1] for s in stated] and layer == [s[2] for s in stated]
    pairs = K.hand_pairs()
    assert verdict[:len(pairs)] == [v for _, _, v, _ in pairs] and all(l is None or l == g for (_, _, _, l), g in zip(pairs, layer))
    assert not got.prb_status.any() and not got.ref_status.any()
    maps, raw = got.map.cpu().numpy(), key_pairs(gpu_device, prb, ref)[4]
    for k in range(len(prb)):
        assert maps[k].tolist() == K.translated(table["pa"][k], table["pb"][k], raw[k]), k
    # law 1: the main layer is the mobile verdict; law 2: plain molecules get the stereo verdict - both on the GPU's own answers
    mobile = S.mobile_identity_batch(ref_d, prb_d).verdict.cpu().tolist()
    stereo = S.stereo_identity_batch(ref_d, prb_d).verdict.cpu().tolist()
    assert stereo == strict
    plain_pairs = 0
    for k, (a, b) in enumerate(zip(prb, ref)):
        assert (verdict[k] in (1, 4, 5, 6)) == (mobile[k] == 1) and (verdict[k] == 0) == (mobile[k] == 0), k
        if K.within_valence(a) and K.within_valence(b) and K.plain(a) and K.plain(b) and not K.fold_made_twins(a, table["pa"][k]) and not K.fold_made_twins(b, table["pb"][k]):
            assert verdict[k] == stereo[k], k
            plain_pairs += 1
    assert plain_pairs >= 200
    assert sum(v == 1 for v in verdict) <= sum(m == 1 for m in mobile)
    # the other way round gives the same verdicts
    back = S.key_identity_batch(prb_d, ref_d)
    assert torch.equal(back.verdict, got.verdict) and torch.equal(back.layer, got.layer)
    # a ref_index: out of the table is invalid; an unusable side is invalid; a side over its budget is undecided
    index = torch.tensor([0, -1, len(ref), 1, 2], device=gpu_device)
    five = (prb_d[0][:5].clone(), prb_d[1][:5].clone())
    five[0][3, SM.TYPE] = 9
    by_index = S.key_identity_batch(ref_d, five, ref_index=index)
    assert by_index.verdict.cpu().tolist() == [verdict[0], K.INVALID, K.INVALID, K.INVALID, K.compare(prb[4], ref[2])["verdict"]]
    assert by_index.ref_status.cpu().tolist() == [0, 3, 3, 0, 0] and by_index.prb_status.cpu().tolist() == [0, 0, 0, 3, 0] and (by_index.map[1:4] == -1).all()
    names = [a for a, *_ in pairs]
    k = names.index("2-pyridone")
    short = S.key_identity_batch((ref_d[0][k:k + 1].contiguous(), ref_d[1][k:k + 1].contiguous()), (prb_d[0][k:k + 1].contiguous(), prb_d[1][k:k + 1].contiguous()),
                                 max_nodes=1)
    assert short.verdict.tolist() == [K.UNDECIDED] and short.layer.tolist() == [-1] and short.prb_status.tolist() == [K.ROW_UNDECIDED]
    hit = S.topk_identity(got.verdict[:len(pairs) // 2 * 2], 2)
    assert hit["hit"].cpu().tolist() == [any(s[0] == 1 for s in stated[i:i + 2]) for i in range(0, len(pairs) // 2 * 2, 2)]
    found = S.key_sites(prb_d[0], prb_d[1].tolist())
    assert isinstance(found, S.KeySites) and torch.equal(found.flags, found.site[..., 0]) and torch.equal(found.mobile_bond, found.masks[:, 7])


# ------------------------------------------------------------------------------------------------------------------ evaluation

PARENT_KEYS = {"rmsd_list", "success_rate", "mean_rmsd", "mean_atom_type_accuracy", "mean_bond_accuracy", "exact_rate", "per_pair", "top_k", "graph",
               "mces", "fingerprint"}


def test_evaluate_reports_the_key_identity(gpu_device, tmp_path, monkeypatch):
    """diffspectra_evaluate(structure_metrics=True) on filler weights, 3 steps, K = 2: with ``cfg.eval.key_identity`` the 'structure' dict
    holds the entry, equal to the mirror on the run's records; without the flag it has the keys it had before.  The Top-1 lies between the
    stereo-aware Top-1 (over pairs without a ring double-bond site) and the mobile Top-1."""
    from diffspectra_amd import filler, evaluate as EV
    from diffspectra_amd.config import qm9s_config
    from diffspectra_amd.dataset_pack import PackedSpectraTable
    from diffspectra_amd.registry import create_model
    from tests.test_structure_metrics_gpu import _graph_dataset
    import diffspectra_amd.dmt  # noqa: F401
    K_, T = 2, 3
    cfg = qm9s_config("ir", device=gpu_device, steps=3, batch_size=4, num_samples=T)
    cfg.eval.begin_ckpt, cfg.eval.end_ckpt, cfg.eval.ckpts, cfg.eval.top_k = 40, 40, "", K_
    table = PackedSpectraTable.from_dataset(_graph_dataset(8, seed=21), "ir", device=gpu_device)
    donor = create_model(cfg)
    donor.eval()
    filler.fill_module_(donor)
    ema = EV.ExponentialMovingAverage(donor.parameters(), decay=0.999)
    (tmp_path / "checkpoints").mkdir()
    EV.save_checkpoint(str(tmp_path / "checkpoints" / "checkpoint_40.pth"), dict(optimizer=None, model=donor, ema=ema, step=7))
    torch.manual_seed(42)
    slot_ds = torch.randperm(8)[:T].repeat_interleave(K_)
    planted = 1 * K_ + 1
    gt_rec, gt_n = table.gt_records.cpu().numpy(), table.num_atom.numpy()
    truth = SM.mol_from_record(gt_rec[int(slot_ds[planted])], gt_n[int(slot_ds[planted])])
    moved = ST.renumbered(truth, np.random.default_rng(13))                    # the ground truth moved and renumbered: its geometry is kept
    gather, kept = shard.gather_by_slot, []

    def gather_and_plant(rec, n_atoms):
        by_slot = gather(rec, n_atoms)
        by_slot[planted] = torch.as_tensor(SM.records([moved])[0][0]).to(by_slot.device)
        kept.append(by_slot)
        return by_slot
    monkeypatch.setattr(shard, "gather_by_slot", gather_and_plant)
    torch.manual_seed(42)
    plain = EV.diffspectra_evaluate(cfg, str(tmp_path), table, structure_metrics=True)[40]["metrics"]["structure"]
    assert set(plain) == PARENT_KEYS
    cfg.eval.key_identity = cfg.eval.mobile_identity = cfg.eval.stereo = True
    torch.manual_seed(42)
    res = EV.diffspectra_evaluate(cfg, str(tmp_path), table, structure_metrics=True)[40]
    monkeypatch.setattr(shard, "gather_by_slot", gather)
    st = res["metrics"]["structure"]
    assert set(st) == PARENT_KEYS | {"key", "mobile", "stereo"}
    entry = st["key"]
    assert set(entry) == {"verdict", "layer", "identity_rate", "strict_rate", "normalised_hits", "mirror", "stereoisomer", "unassigned", "undecided", "invalid",
                          "sites", "top_k"}
    gen_rec = kept[-1].cpu().numpy()
    gen_n = np.array([len(atom) for _, atom, _, _ in res["processed_mols"]], np.int32)
    gen = [SM.mol_from_record(gen_rec[s], gen_n[s]) for s in range(len(slot_ds))]
    gts = [SM.mol_from_record(gt_rec[int(r)], gt_n[int(r)]) for r in slot_ds]
    stated = [K.identity(a, b) for a, b in zip(gen, gts)]
    assert entry["verdict"].cpu().tolist() == [s[0] for s in stated] and entry["layer"].cpu().tolist() == [s[2] for s in stated]
    assert stated[planted][0] in (K.IDENTICAL, K.UNASSIGNED), "the same normal form in the same geometry: identical, unless a site is too flat"
    count = lambda code: sum(s[0] == code for s in stated)
    assert entry["identity_rate"] == count(1) / len(stated) and entry["strict_rate"] == st["stereo"]["identity_rate"]
    assert entry["normalised_hits"] == sum(s[2] == 1 for s in stated)
    assert (entry["mirror"], entry["stereoisomer"], entry["unassigned"], entry["undecided"], entry["invalid"]) == (count(4), count(5), count(6), count(2), count(3))
    hits = [any(s[0] == 1 for s in stated[i:i + K_]) for i in range(0, len(stated), K_)]
    assert entry["top_k"]["hit"].cpu().tolist() == hits and float(entry["top_k"]["acc_at_k"]) == sum(hits) / T
    # the Top-1 is at most the mobile Top-1 and at least the stereo-aware Top-1 over the pairs without a ring double-bond site
    assert entry["identity_rate"] <= st["mobile"]["identity_rate"]
    ring_site = [any(K._ring_bond(ST._bonds(m).tolist(), s["a"], s["b"]) for s in ST.perceive(m)["ez"]) for m in gts]
    strict_hits = [v == 1 and not ring for v, ring in zip(st["stereo"]["verdict"].cpu().tolist(), ring_site)]
    assert sum(strict_hits) <= count(1)
    assert all(s[0] == 1 for s, hit in zip(stated, strict_hits) if hit)
