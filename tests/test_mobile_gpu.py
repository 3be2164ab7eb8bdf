"""GPU: ``dsm_mobile_records`` and ``dsm_normal_records`` (csrc/ds_mobile.hip) and what ``structure_metrics`` and ``evaluate`` build on them
against the plain-Python mirror of tests/mobile_mirror.py, which is written from include/diffspectra_mobile.h and pinned to hand-stated
expectations by tests/test_mobile_cpu.py.  Every output is an integer or a byte and is compared exactly."""
import numpy as np
import pytest
import torch

from diffspectra_amd import engine as E, shard, structure_metrics as S
from tests import graph_mirror as GM, mobile_mirror as M, structure_mirror as SM
from tests.helpers import to_dev
from tests.test_scaffold_cpu import same_partition
from tests.test_valence_gpu import random_records

pytestmark = pytest.mark.gpu

GUARD_ROWS = 3
MOBILE_DTYPES = [torch.uint8, torch.int8, torch.uint8, torch.uint8, torch.int32, torch.int32, torch.uint8]
NORMAL_DTYPES = [torch.uint8, torch.int32, torch.uint8, torch.uint8]


def on(dev, rec, n):
    return to_dev(dev, rec, torch.uint8), to_dev(dev, n, torch.int32)


def gpu_mobile(dev, rec, n, max_nodes=None):
    out = [t.cpu() for t in E.mobile_records(*on(dev, rec, n), max_nodes)]
    assert [t.dtype for t in out] == MOBILE_DTYPES
    assert [tuple(t.shape) for t in out] == [(len(n), 29), (len(n), 29), (len(n), 29), (len(n), 14), (len(n), 4), (len(n),), (len(n),)]
    return [t.numpy() for t in out]


def gpu_normal(dev, rec, n, max_nodes=None):
    out = [t.cpu() for t in E.normal_records(*on(dev, rec, n), max_nodes)]
    assert [t.dtype for t in out] == NORMAL_DTYPES
    assert [tuple(t.shape) for t in out] == [(len(n), E.RECORD_BYTES), (len(n),), (len(n), 29), (len(n),)]
    return [t.numpy() for t in out]


def same_arrays(got, want, keys):
    for key, g, w in zip(keys, got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (key, g.shape, w.shape, g.dtype, w.dtype)
        rows = np.nonzero((g != w).reshape(len(g), -1).any(1))[0]
        assert rows.size == 0, (key, rows[:5].tolist(), g[rows[0]].tolist(), w[rows[0]].tolist())


def both_against_the_mirror(dev, rec, n, max_nodes=None):
    """Every output of both entry points against the mirror; returns (mobile arrays, normal arrays) of the GPU."""
    budget = M.DEFAULT_NODES if max_nodes is None else max_nodes
    mobile, normal = gpu_mobile(dev, rec, n, max_nodes), gpu_normal(dev, rec, n, max_nodes)
    same_arrays(mobile, M.as_arrays(M.analyse_table(rec, n, budget)), M.KEYS)
    same_arrays(normal, M.normal_table(rec, n, budget), M.NORMAL_KEYS)
    return mobile, normal


@pytest.fixture(scope="module")
def molecules():
    """The table, three renumberings of each of its molecules (with the permutations) and the corpus as one record table: computed once,
    shared, never changed."""
    rows = M.hand_table()
    rng = np.random.default_rng(23)
    table = [mol for _, mol, _ in rows]
    perms, renumbered = [], []
    for mol in table:
        for _ in range(3):
            perm = rng.permutation(len(mol["type"]))                            # new atom i is old atom perm[i]
            perms.append(perm)
            renumbered.append(M.renumbered(mol, perm))
    corpus = M.corpus()
    mols = table + renumbered + corpus
    rec, n = SM.records(mols)
    return dict(rows=rows, perms=perms, mols=mols, rec=rec, n=n, corpus=slice(len(n) - len(corpus), len(n)))


# ------------------------------------------------------------------------------------------------------------------ the kernels

def test_table_renumberings_and_corpus_against_the_mirror(gpu_device, molecules):
    rows, perms, rec, n = (molecules[k] for k in ("rows", "perms", "rec", "n"))
    assert 300 <= len(n) <= 500
    mobile, normal = both_against_the_mirror(gpu_device, rec, n)
    fixed_h, q_res, group_of, group_h, summary, nodes, status = mobile
    assert not status.any() and not normal[3].any()
    # ... and so the hand-stated table holds for the kernel, under renumbering too
    T = len(rows)
    for k, (name, mol, stated) in enumerate(rows):
        heavy = len(stated["fixed_h"])
        groups = lambda p: sorted(sorted(np.nonzero(group_of[p] == g)[0].tolist()) for g in range(summary[p, 1]))
        assert fixed_h[k, :heavy].tolist() == stated["fixed_h"] and q_res[k, :heavy].tolist() == stated["q_res"], name
        assert groups(k) == stated["groups"] and group_h[k, :len(stated["groups"])].tolist() == stated["group_h"], name
        assert summary[k].tolist() == [heavy, len(stated["groups"]), sum(stated["group_h"]), stated["p"]], name
        for j in range(3):
            p, perm = T + 3 * k + j, perms[3 * k + j]
            new = {int(old): i for i, old in enumerate(perm)}
            assert fixed_h[p].tolist() == M.moved(fixed_h[k].tolist(), perm, 0xff) and q_res[p].tolist() == M.moved(q_res[k].tolist(), perm, 0), name
            assert groups(p) == sorted(sorted(new[a] for a in g) for g in stated["groups"]) and summary[p].tolist() == summary[k].tolist(), name
    # the ground the comparison stands on (asserted on the mirror in tests/test_mobile_cpu.py)
    part = summary[molecules["corpus"]]
    assert 4 * int((part[:, 1] > 0).sum()) >= len(part) and int(nodes.max()) >= 3 and int((summary[:, 3] != 0).sum()) >= 4 and int(q_res.any(1).sum()) >= 4
    # the rows as records: symmetric bond bytes of 0 and 1, nothing behind the bond block, group and proton nodes after the kept atoms
    bonds = normal[0][:, SM.BOND:SM.BOND_END].reshape(-1, 29, 29)
    assert np.array_equal(bonds, bonds.transpose(0, 2, 1)) and int(bonds.max()) == 1 and not normal[0][:, SM.BOND_END:].any()
    assert set(np.unique(normal[0][:, SM.TYPE:SM.FC]).tolist()) == {0, 1, 2, 3, 4, M.GROUP_TYPE, M.PROTON_TYPE}
    assert np.array_equal(normal[1], summary[:, 0] + summary[:, 1] + (summary[:, 3] != 0))


def test_sizes_garbage_unusable_and_the_hard_shapes(gpu_device, molecules):
    rng = np.random.default_rng(20261020)
    sizes = np.array([0, 1, 2, 3, 28, 29, 40, -3] * 16, np.int32)
    rec, n, clean = random_records(rng, len(sizes), garbage=True, sizes=sizes)
    rec[5::8, SM.TYPE + 3] = 5                                                   # every 29-atom record of the first kind: a type byte above 4
    clean[5::8, SM.TYPE + 3] = 5
    mobile, normal = both_against_the_mirror(gpu_device, rec, n)
    assert set(mobile[6].tolist()) == {M.OK, M.UNUSABLE} and int((mobile[6] == M.OK).sum()) >= 60
    unusable = mobile[6] == M.UNUSABLE
    assert (mobile[0][unusable] == 0xff).all() and not mobile[4][unusable].any() and not normal[0][unusable].any() and not normal[1][unusable].any()
    same_arrays(gpu_mobile(gpu_device, clean, n), mobile, M.KEYS)                # what is ignored is ignored
    same_arrays(gpu_normal(gpu_device, clean, n), normal, M.NORMAL_KEYS)
    # 29 kept atoms and a group: the analysis answers, the normal form would have 30 nodes; 28 kept atoms and a group fit; with a proton
    # node on top they do not; the 29-atom chain, ring and complete graph; sparse random graphs of 29 atoms
    amide = lambda k: GM.molecule([1] * (k - 2) + [3, 2], [(i, i + 1) for i in range(k - 3)] + [(k - 3, k - 2), (k - 3, k - 1)],
                                  orders=[1] * (k - 3) + [2, 1])
    charged = amide(28)
    charged["fc"] = charged["fc"].copy()
    charged["type"] = charged["type"].copy()
    charged["type"][0], charged["fc"][0] = 2, 1                                  # an ammonium end: p = 1
    hard = [amide(29), amide(28), charged, GM.carbons(29, [(i, i + 1) for i in range(28)]), GM.carbons(29, [(i, (i + 1) % 29) for i in range(29)]), GM.k29()]
    rec, n = SM.records(hard + [GM.random_molecule(rng, 29) for _ in range(20)])
    mobile, normal = both_against_the_mirror(gpu_device, rec, n)
    assert mobile[4][:3].tolist() == [[29, 1, 2, 0], [28, 1, 2, 0], [28, 1, 2, 1]] and mobile[6][:3].tolist() == [0, 0, 0]
    assert normal[3][:6].tolist() == [M.OVERFLOW, M.OK, M.OVERFLOW, M.OK, M.OK, M.OK] and normal[1][:6].tolist() == [0, 29, 0, 29, 29, 29]
    assert not normal[0][0].any() and (normal[2][0] == 0xff).all() and normal[0][1][SM.TYPE + 28] == M.GROUP_TYPE


def test_a_budget_of_one_node_is_undecided_where_the_mirror_says_so(gpu_device, molecules):
    rec, n = molecules["rec"], molecules["n"]
    mobile, normal = both_against_the_mirror(gpu_device, rec, n, 1)
    undecided = mobile[6] == M.UNDECIDED
    assert 30 <= int(undecided.sum()) <= len(n) - 100 and set(mobile[6].tolist()) == {M.OK, M.UNDECIDED}
    assert (mobile[0][undecided] == 0xff).all() and not mobile[5][undecided].any() and not normal[1][undecided].any()
    names = [name for name, *_ in molecules["rows"]]
    assert mobile[6][names.index("2-pyridone")] == M.OK and mobile[6][names.index("2-hydroxypyridine, N-C(OH)")] == M.UNDECIDED
    both_against_the_mirror(gpu_device, rec[:60], n[:60], 2)
    both_against_the_mirror(gpu_device, rec[:60], n[:60], E.MOBILE_MAX_NODES)


def test_guarded_outputs_repeat_runs_batch_independence_and_no_records(gpu_device, molecules):
    """Every output of both kernels between guard rows filled with a pattern (P = 65: a workgroup with three waves that have no record); two
    runs bit-identical; a row's outputs do not depend on the batch around it; P = 0."""
    rng = np.random.default_rng(9)
    P = 65
    rows = rng.permutation(len(molecules["n"]))[:P]
    rec_d, n_d = on(gpu_device, molecules["rec"][rows], molecules["n"][rows])
    lib, stream = E.load_library(), torch.cuda.current_stream().cuda_stream

    def guarded(count, width, dtype):
        raw = torch.full((count + 2 * GUARD_ROWS, width), 0x5A, dtype=torch.uint8, device=gpu_device).view(dtype)
        return raw, raw[GUARD_ROWS:GUARD_ROWS + count]

    def intact(raw):
        b = raw.view(torch.uint8)
        return bool((b[:GUARD_ROWS] == 0x5A).all()) and bool((b[-GUARD_ROWS:] == 0x5A).all())
    for budget in (M.DEFAULT_NODES, 1):
        bufs = [guarded(P, 29, torch.uint8), guarded(P, 29, torch.int8), guarded(P, 29, torch.uint8), guarded(P, 14, torch.uint8),
                guarded(P, 16, torch.int32), guarded(P, 4, torch.int32), guarded(P, 1, torch.uint8)]
        st = lib.dsm_mobile_records(rec_d.data_ptr(), n_d.data_ptr(), P, budget, *(view.data_ptr() for _, view in bufs), stream)
        torch.cuda.synchronize()
        assert st == 0 and all(intact(raw) for raw, _ in bufs)
        plain, again = E.mobile_records(rec_d, n_d, budget), E.mobile_records(rec_d, n_d, budget)
        assert all(torch.equal(view.reshape(t.shape), t) and torch.equal(t, u) for (_, view), t, u in zip(bufs, plain, again))
        outs = [guarded(P, E.RECORD_BYTES, torch.uint8), guarded(P, 4, torch.int32), guarded(P, 29, torch.uint8), guarded(P, 1, torch.uint8)]
        st = lib.dsm_normal_records(rec_d.data_ptr(), n_d.data_ptr(), P, budget, *(view.data_ptr() for _, view in outs), stream)
        torch.cuda.synchronize()
        assert st == 0 and all(intact(raw) for raw, _ in outs)
        forms, forms_again = E.normal_records(rec_d, n_d, budget), E.normal_records(rec_d, n_d, budget)
        assert all(torch.equal(view.reshape(t.shape), t) and torch.equal(t, u) for (_, view), t, u in zip(outs, forms, forms_again))
        for sub in ([64], [5], [17, 64, 5, 0]):
            idx = torch.tensor(sub, device=gpu_device)
            alone = E.mobile_records(rec_d[idx].contiguous(), n_d[idx].contiguous(), budget) + E.normal_records(rec_d[idx].contiguous(), n_d[idx].contiguous(), budget)
            assert all(torch.equal(s, t[idx]) for s, t in zip(alone, plain + forms))
    assert int((plain[6] == M.UNDECIDED).sum()) >= 3
    assert [a.shape[0] for a in gpu_mobile(gpu_device, molecules["rec"][:0], molecules["n"][:0])] == [0] * 7
    assert [a.shape[0] for a in gpu_normal(gpu_device, molecules["rec"][:0], molecules["n"][:0])] == [0] * 4
    # the library's own argument checks, in the header's order: the budget, P, NULL, alignment; P = 0 before the pointers
    args = [view.data_ptr() for _, view in outs]
    call = lambda rec_p, n_p, count, budget, first: lib.dsm_normal_records(rec_p, n_p, count, budget, first, *args[1:], stream)
    assert call(0, 0, 0, 1, 0) == 0 and call(0, 0, 0, 0, 0) == -1 and call(rec_d.data_ptr(), n_d.data_ptr(), -1, 1, args[0]) == -1
    assert call(rec_d.data_ptr(), n_d.data_ptr(), P, E.MOBILE_MAX_NODES + 1, args[0]) == -1 and call(0, n_d.data_ptr(), P, 1, args[0]) == -1
    assert call(rec_d.data_ptr(), n_d.data_ptr(), P, 1, 0) == -1 and call(rec_d.data_ptr() + 1, n_d.data_ptr(), 1, 1, args[0]) == -1
    assert call(rec_d.data_ptr(), n_d.data_ptr(), 1, 1, args[0] + 2) == -1
    assert lib.dsm_mobile_records(rec_d.data_ptr(), n_d.data_ptr(), P, 1, *(view.data_ptr() for _, view in bufs[:6]), 0, stream) == -1
    torch.cuda.synchronize()
    assert all(intact(raw) for raw, _ in outs + bufs)


# ------------------------------------------------------------------------------------------------------------------ the public interface

def check_map(prb, ref, image):
    """``image``: original kept atom of ``ref`` for every original atom of ``prb``, -1 elsewhere - a bijection of the kept atoms that keeps the
    element, the fixed hydrogens, the residual charge, the skeleton and the groups."""
    (a_rec, a_n), (b_rec, b_n) = SM.records([prb]), SM.records([ref])
    A, B = M.Analysis(a_rec[0], a_n[0]), M.Analysis(b_rec[0], b_n[0])
    image = [int(x) for x in image]
    assert [i for i, x in enumerate(image) if x >= 0] == A.kept and sorted(image[i] for i in A.kept) == B.kept
    for i in A.kept:
        j = image[i]
        assert (A.types[i], A.fixed[i], A.q_res[i]) == (B.types[j], B.fixed[j], B.q_res[j])
        assert sorted(image[k] for k in A.nbrs[i]) == B.nbrs[j]
        assert (i in A.group_of) == (j in B.group_of)
        if i in A.group_of:
            assert sorted(image[k] for k in A.groups[A.group_of[i]]) == B.groups[B.group_of[j]]


def test_mobile_identity_against_the_hand_pairs_and_the_graph_mirror(gpu_device, molecules):
    pairs = M.hand_pairs()
    prb, ref = [M.named(a) for a, *_ in pairs], [M.named(b) for _, b, *_ in pairs]
    # the corpus against itself renumbered, against one shifted form where there is one, and against its neighbour
    rng = np.random.default_rng(5)
    corpus = molecules["mols"][molecules["corpus"]][1::3]                       # (molecules grown on a conjugated chain: mobile_mirror.corpus)
    for k, mol in enumerate(corpus):
        A = M.Analysis(*[x[0] for x in SM.records([mol])])
        other = next((s for s in (M.shifted(mol, p) for p in A.paths) if s is not None), None)
        prb += [GM.permuted(mol, rng), mol] + ([other] if other is not None else [])
        ref += [mol, corpus[(k + 1) % len(corpus)]] + ([mol] if other is not None else [])
    stated = [M.identity(a, b) for a, b in zip(prb, ref)]
    assert [s[0] for s in stated[:len(pairs)]] == [v for *_, v, _ in pairs] and [s[2] for s in stated[:len(pairs)]] == [layer for *_, layer in pairs]
    assert sum(s[2] == 1 for s in stated[len(pairs):]) >= 15 and sum(s[0] == M.DIFFERENT for s in stated[len(pairs):]) >= 40
    prb_d, ref_d = on(gpu_device, *SM.records(prb)), on(gpu_device, *SM.records(ref))
    got = S.mobile_identity_batch(ref_d, prb_d)
    assert isinstance(got, S.MobileIdentity) and [t.dtype for t in got] == [torch.uint8, torch.uint8, torch.int8, torch.int32, torch.uint8, torch.uint8, torch.int32]
    assert got.verdict.cpu().tolist() == [s[0] for s in stated] and got.strict.cpu().tolist() == [s[1] for s in stated]
    assert got.layer.cpu().tolist() == [s[2] for s in stated] and not got.prb_status.any() and not got.ref_status.any()
    maps = got.map.cpu().numpy()
    for k, s in enumerate(stated):
        if s[0] == M.IDENTICAL:
            check_map(prb[k], ref[k], maps[k][:len(prb[k]["type"])])
            assert (maps[k][len(prb[k]["type"]):] == -1).all()
        else:
            assert (maps[k] == -1).all()
    # the other way round gives the same verdicts
    back = S.mobile_identity_batch(prb_d, ref_d)
    assert torch.equal(back.verdict, got.verdict) and torch.equal(back.layer, got.layer)
    # a ref_index: out of the table is invalid; an unusable side is invalid; a side over its budget or over 29 nodes is undecided
    index = torch.tensor([0, -1, len(ref), 1, 2], device=gpu_device)
    five = (prb_d[0][:5].clone(), prb_d[1][:5].clone())
    five[0][3, SM.TYPE] = 9
    by_index = S.mobile_identity_batch(ref_d, five, ref_index=index)
    assert by_index.verdict.cpu().tolist() == [got.verdict[0].item(), M.INVALID, M.INVALID, M.INVALID, M.identity(prb[4], ref[2])[0]]
    assert by_index.ref_status.cpu().tolist() == [0, 3, 3, 0, 0] and by_index.prb_status.cpu().tolist() == [0, 0, 0, 3, 0] and (by_index.map[1:4] == -1).all()
    names = [a for a, *_ in pairs]
    k = names.index("2-pyridone")                                               # against 2-hydroxypyridine, N-C(OH): three nodes on that side
    short = S.mobile_identity_batch((ref_d[0][k + 1:k + 2].contiguous(), ref_d[1][k + 1:k + 2].contiguous()),
                                    (prb_d[0][k + 1:k + 2].contiguous(), prb_d[1][k + 1:k + 2].contiguous()), max_nodes=1)
    assert short.verdict.tolist() == [M.PAIR_UNDECIDED] and short.layer.tolist() == [-1] and short.ref_status.tolist() == [M.UNDECIDED]
    hit = S.topk_identity(got.verdict[:len(pairs) // 2 * 2], 2)
    assert hit["hit"].cpu().tolist() == [any(s[0] == 1 for s in stated[i:i + 2]) for i in range(0, len(pairs) // 2 * 2, 2)]


def test_mobile_hydrogens_normal_forms_and_classes(gpu_device, molecules):
    rec, n, mols = molecules["rec"], molecules["n"], molecules["mols"]
    rec_d = to_dev(gpu_device, rec, torch.uint8)
    found = S.mobile_hydrogens(rec_d, n.tolist())
    assert isinstance(found, S.MobileHydrogens) and found.fixed_h.device.type == gpu_device.type and bool(found.ok.all())
    want = M.as_arrays(M.analyse_table(rec, n))
    assert found.n_groups.cpu().tolist() == want[4][:, 1].tolist() and found.proton_balance.cpu().tolist() == want[4][:, 3].tolist()
    forms = S.normal_form_records(rec_d, n.tolist())
    same_arrays([t.cpu().numpy() for t in forms], M.normal_table(rec, n), M.NORMAL_KEYS)
    # graph_mirror on the mirror's normal forms: the hash and the classes
    rows = np.concatenate([np.arange(len(molecules["rows"]) * 4), np.arange(len(n))[molecules["corpus"]][::4]])
    normal = [M.normal_mol(mols[int(r)])[0] for r in rows]
    sub = (forms[0][to_dev(gpu_device, rows, torch.int64)].contiguous(), forms[1][to_dev(gpu_device, rows, torch.int64)].contiguous())
    assert [h & GM.MASK for h in E.graph_hash_records(*sub).cpu().tolist()] == [GM.graph_hash(m) for m in normal]
    cls = S.mobile_classes(rec_d[to_dev(gpu_device, rows, torch.int64)].contiguous(), n[rows].tolist()).cpu().tolist()
    stated = M.classes([mols[int(r)] for r in rows])
    assert cls == stated and same_partition(cls, stated) and len(set(cls)) < len(molecules["rows"]) + len(rows) - len(molecules["rows"]) * 4
    # rows without a normal form are classes of their own
    two = rec_d[:4].clone()
    two[1, SM.TYPE], two[3, SM.TYPE] = 9, 9
    assert S.mobile_classes(two, n[:4].tolist()).cpu().tolist() == [0, 1, S.mobile_classes(rec_d[:4].contiguous(), n[:4].tolist())[2].item(), 3]


# ------------------------------------------------------------------------------------------------------------------ evaluation

PARENT_KEYS = {"rmsd_list", "success_rate", "mean_rmsd", "mean_atom_type_accuracy", "mean_bond_accuracy", "exact_rate", "per_pair", "top_k", "graph",
               "mces", "fingerprint"}


def test_evaluate_reports_the_mobile_identity(gpu_device, tmp_path, monkeypatch):
    """diffspectra_evaluate(structure_metrics=True) on filler weights, 3 steps, K = 2: with ``cfg.eval.mobile_identity`` the 'structure' dict
    holds the entry, equal to the mirror on the run's records; without the flag it has the keys it had before."""
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
    moved = GM.permuted(SM.mol_from_record(gt_rec[int(slot_ds[planted])], gt_n[int(slot_ds[planted])]), np.random.default_rng(13))
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
    cfg.eval.mobile_identity = True
    torch.manual_seed(42)
    res = EV.diffspectra_evaluate(cfg, str(tmp_path), table, structure_metrics=True)[40]
    monkeypatch.setattr(shard, "gather_by_slot", gather)
    st = res["metrics"]["structure"]
    assert set(st) == PARENT_KEYS | {"mobile"}
    entry = st["mobile"]
    assert set(entry) == {"verdict", "layer", "identity_rate", "strict_rate", "normalised_hits", "undecided", "invalid", "top_k"}
    gen_rec = kept[-1].cpu().numpy()
    gen_n = np.array([len(atom) for _, atom, _, _ in res["processed_mols"]], np.int32)
    stated = [M.identity(SM.mol_from_record(gen_rec[s], gen_n[s]), SM.mol_from_record(gt_rec[int(r)], gt_n[int(r)])) for s, r in enumerate(slot_ds)]
    assert entry["verdict"].cpu().tolist() == [s[0] for s in stated] and entry["layer"].cpu().tolist() == [s[2] for s in stated]
    assert stated[planted][0] == M.IDENTICAL and stated[planted][2] == 0
    assert entry["identity_rate"] == sum(s[0] == 1 for s in stated) / len(stated) and entry["strict_rate"] == st["graph"]["identity_rate"]
    assert entry["normalised_hits"] == sum(s[2] == 1 for s in stated) and entry["undecided"] == sum(s[0] == 2 for s in stated)
    hits = [any(s[0] == 1 for s in stated[i:i + K_]) for i in range(0, len(stated), K_)]
    assert entry["top_k"]["hit"].cpu().tolist() == hits and hits[1] and float(entry["top_k"]["acc_at_k"]) == sum(hits) / T
