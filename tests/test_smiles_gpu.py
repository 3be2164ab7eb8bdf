"""GPU: ``dsl_smiles_records`` (csrc/ds_smiles.hip) and what ``structure_metrics`` and ``evaluate`` build on it against the plain-Python mirror of
tests/smiles_mirror.py, which is written from include/diffspectra_smiles.h and pinned by tests/test_smiles_cpu.py.  Every output is a byte or an
integer and is compared exactly."""
import numpy as np
import pytest
import torch

from diffspectra_amd import engine as E, shard, structure_metrics as S
from tests import graph_mirror as GM, smiles_mirror as L, structure_mirror as SM
from tests.helpers import to_dev
from tests.test_valence_gpu import random_records

pytestmark = pytest.mark.gpu

GUARD_ROWS = 3
TABLE = 257                          # rows per launch: 64 full workgroups and one with a single record


def on(dev, rec, n):
    return to_dev(dev, rec, torch.uint8), to_dev(dev, n, torch.int32)


def gpu_rows(dev, rec, n, max_nodes=4096, table=TABLE):
    """``smiles_records`` in launches of ``table`` rows as the mirror's list of row dicts."""
    rows = []
    for at in range(0, len(n), table):
        out = [t.cpu() for t in E.smiles_records(*on(dev, rec[at:at + table], n[at:at + table]), max_nodes)]
        P = len(n[at:at + table])
        assert [t.dtype for t in out] == [torch.uint8, torch.int32, torch.uint8, torch.int32, torch.int32]
        assert [tuple(t.shape) for t in out] == [(P, 384), (P,), (P,), (P,), (P, 29)]
        text, length, status, nodes, order = (t.numpy() for t in out)
        for p in range(P):
            assert not text[p, length[p]:].any(), (at + p, "bytes after the text")
            rows.append(dict(text=text[p, :length[p]].tobytes(), length=int(length[p]), status=int(status[p]), nodes=int(nodes[p]), atom_order=order[p].tolist()))
    return rows


def same_rows(got, want):
    assert len(got) == len(want)
    for p, (g, w) in enumerate(zip(got, want)):
        assert g == w, (p, {k: (g[k], w[k]) for k in L.KEYS if g[k] != w[k]})


def dirty(rec, n, rng):
    """The same molecules with NaN-filled positions and random bytes in everything the contract says is ignored: atoms >= n, the lower triangle,
    the diagonal and the pad."""
    out = rec.copy()
    out[:, :SM.TYPE] = 0xFF
    out[:, SM.BOND_END:] = rng.integers(0, 256, size=out[:, SM.BOND_END:].shape)
    for p in range(len(n)):
        k = int(min(max(int(n[p]), 0), 29))
        out[p, SM.TYPE + k:SM.FC] = rng.integers(0, 256, size=29 - k)
        out[p, SM.FC + k:SM.BOND] = rng.integers(0, 256, size=29 - k)
        bond = out[p, SM.BOND:SM.BOND_END].reshape(29, 29)
        noise = rng.integers(0, 256, size=(29, 29)).astype(np.uint8)
        ignored = np.tril(np.ones((29, 29), bool))
        ignored[k:, :] = True
        ignored[:, k:] = True
        bond[ignored] = noise[ignored]
    return out


@pytest.fixture(scope="module")
def molecules():
    """The forced table, the property molecules, both sides of the 2000 seeded pairs and a renumbered copy of every seeded ground truth as one
    record table with the mirror's rows: computed once, shared, never changed."""
    rng = np.random.default_rng(20261022)
    named = [m for _, m in L.forced_table()] + [m for _, m in L.property_molecules()]
    ref, prb, _ = GM.seeded_pairs(2000)
    moved = [GM.permuted(m, rng) for m in ref]
    ref_rows, prb_rows = L.seeded_rows(2000)
    mols = named + list(ref) + list(prb) + moved
    want = [L.write(m) for m in named] + ref_rows + prb_rows + [L.write(m) for m in moved]
    rec, n = SM.records(mols)
    return dict(mols=mols, rec=rec, n=n, want=want, named=len(named), ref=slice(len(named), len(named) + 2000),
                prb=slice(len(named) + 2000, len(named) + 4000), moved=slice(len(named) + 4000, len(named) + 6000))


@pytest.fixture(scope="module")
def table(gpu_device, molecules):
    """The kernel's rows of the whole table, in launches of 257 rows."""
    return gpu_rows(gpu_device, molecules["rec"], molecules["n"])


# ------------------------------------------------------------------------------------------------------------------ the kernel

def test_table_against_the_mirror(molecules, table):
    same_rows(table, molecules["want"])
    assert sorted({int(k) for k in molecules["n"][molecules["ref"]]}) == list(range(3, 30))
    for (text, _), got in zip(L.forced_table(), table):
        assert got["text"] == text.encode() and got["status"] == L.OK
    # a renumbered molecule gets the same string; its atoms land where the renumbering says
    for a, b in zip(table[molecules["ref"]], table[molecules["moved"]]):
        assert (a["text"], a["status"], a["nodes"]) == (b["text"], b["status"], b["nodes"])
    statuses = [g["status"] for g in table]
    assert statuses.count(L.OVERFLOW) == 1 and statuses.count(L.OK) == len(table) - 1


def test_nodes_are_zero_exactly_where_refinement_alone_is_discrete(molecules, table):
    discrete = [L.refinement_is_discrete(m) for m in molecules["mols"]]
    assert [g["nodes"] == 0 for g in table] == discrete and 0.05 < 1 - sum(discrete) / len(discrete) < 0.5


def test_atom_order_is_an_isomorphism_onto_the_parsed_string(molecules, table):
    checked = 0
    for k in list(range(molecules["named"])) + list(range(molecules["named"], len(table), 9)):
        got, mol = table[k], molecules["mols"][k]
        if got["status"] == L.OVERFLOW:
            continue
        back = L.parse(got["text"].decode("ascii"))
        assert GM.is_isomorphism(mol, back, L.expanded_order(mol, got["atom_order"])), k
        atoms, _, _ = L.written_graph(mol)
        assert sorted(got["atom_order"][i] for i in atoms) == list(range(back["string_atoms"])), k
        checked += 1
    assert checked > 600


def test_guarded_outputs_garbage_repeat_runs_and_batch_independence(gpu_device, molecules):
    """Every output between guard rows filled with a pattern (P = 65: a workgroup with three waves that have no record), on records whose
    ignored bytes are garbage; two runs bit-identical; a row's outputs do not depend on the batch around it."""
    rng = np.random.default_rng(9)
    P = 65
    rows = np.concatenate([rng.permutation(len(molecules["n"]))[:P - 12], np.arange(molecules["named"])[-12:]])
    rec, n = dirty(molecules["rec"][rows], molecules["n"][rows], rng), molecules["n"][rows]
    rec_d, n_d = on(gpu_device, rec, n)
    lib, stream = E.load_library(), torch.cuda.current_stream().cuda_stream

    def guarded(width, dtype):
        raw = torch.full((P + 2 * GUARD_ROWS, width), 0x5A, dtype=torch.uint8, device=gpu_device).view(dtype)
        return raw, raw[GUARD_ROWS:GUARD_ROWS + P]

    def intact(raw):
        b = raw.view(torch.uint8)
        return bool((b[:GUARD_ROWS] == 0x5A).all()) and bool((b[-GUARD_ROWS:] == 0x5A).all())
    bufs = [guarded(384, torch.uint8), guarded(4, torch.int32), guarded(1, torch.uint8), guarded(4, torch.int32), guarded(116, torch.int32)]
    st = lib.dsl_smiles_records(rec_d.data_ptr(), n_d.data_ptr(), P, 4096, *(view.data_ptr() for _, view in bufs), stream)
    torch.cuda.synchronize()
    assert st == 0 and all(intact(raw) for raw, _ in bufs)
    plain, again = E.smiles_records(rec_d, n_d), E.smiles_records(rec_d, n_d)
    assert all(torch.equal(view.reshape(t.shape), t) and torch.equal(t, u) for (_, view), t, u in zip(bufs, plain, again))
    same_rows(gpu_rows(gpu_device, rec, n), [molecules["want"][r] for r in rows])          # what is ignored is ignored, every byte is defined
    for sub in ([64], [5], [17, 64, 5, 0]):
        idx = torch.tensor(sub, device=gpu_device)
        alone = E.smiles_records(rec_d[idx].contiguous(), n_d[idx].contiguous())
        assert all(torch.equal(s, t[idx]) for s, t in zip(alone, plain))
    assert gpu_rows(gpu_device, rec[:0], n[:0]) == []


def test_edge_rows(gpu_device):
    rng = np.random.default_rng(20261023)
    # unusable rows of each kind, and the same bytes where they are not looked at
    base, n = SM.records([L.glycine_zwitterion()] * 7)
    count = int(n[0])
    base[0, SM.TYPE + count - 1] = 5
    base[1, SM.BOND + 1 * 29 + 4] = 4
    n[2], n[3] = 0, -7
    base[4, SM.BOND + 4 * 29 + 1] = 4
    base[5, SM.BOND + 28 * 29 + 28] = 9
    base[6, SM.TYPE + count] = 77
    base[6, SM.BOND + 2 * 29 + count + 1] = 200
    got = gpu_rows(gpu_device, base, n)
    none = dict(text=b"", length=0, status=L.UNUSABLE, nodes=0, atom_order=[-1] * 29)
    assert got[:4] == [none] * 4 and got[4:] == [L.write(L.glycine_zwitterion())] * 3 and got == L.write_table(base, n)
    # sizes at which paths change, clamped counts, dense random graphs with garbage: long strings, two-digit ring numbers, overflows
    sizes = np.array([1, 2, 28, 29, 28, 29, 40, -3] * 6, np.int32)
    rec, n, clean = random_records(rng, len(sizes), garbage=True, sizes=sizes)
    want = L.write_table(rec, n)
    got = gpu_rows(gpu_device, rec, n)
    same_rows(got, want)
    assert gpu_rows(gpu_device, clean, n) == got
    assert {w["status"] for w in want} >= {L.OK, L.OVERFLOW, L.UNUSABLE} and any(b"%1" in w["text"] for w in want) and max(w["length"] for w in want) > 128
    # hydrogen counts and charges of two and three digits
    odd = [L._with_h([1], [], [], [12]), L._with_h([2, 3, 4, 1], [(0, 1), (1, 2), (2, 3)], [1, 1, 1], [0, 0, 0, 10], [127, -128, -100, 10]),
           L._with_h([0, 0], [(0, 1)], [2], [0, 0], [0, -1])]
    rec, n = SM.records(odd)
    got = gpu_rows(gpu_device, rec, n)
    assert got == L.write_table(rec, n) and got[0]["text"] == b"[CH12]" and b"[N+127]" in got[1]["text"] and b"[O-128]" in got[1]["text"]
    assert b"[F-100]" in got[1]["text"] and b"[CH10+10]" in got[1]["text"] and got[2]["text"] in (b"[H]=[H-]", b"[H-]=[H]")
    # K29, the budget, the empty table
    rec, n = SM.records([GM.k29(), L.cubane(), L.propane()])
    got = gpu_rows(gpu_device, rec, n, max_nodes=0)
    assert got == L.write_table(rec, n, 0)
    assert (got[0]["status"], got[0]["nodes"], got[0]["length"]) == (L.OVERFLOW, 28, 0)
    assert got[1]["status"] == L.UNCERTIFIED and got[2]["status"] == L.OK and got[2]["text"] == b"C(C)C"
    back = L.parse(got[1]["text"].decode())
    assert GM.same_graph({k: back[k] for k in ("type", "fc", "bond")}, L.cubane())
    for budget in (1, 5, 79, 80):
        assert gpu_rows(gpu_device, rec[1:2], n[1:2], max_nodes=budget) == L.write_table(rec[1:2], n[1:2], budget)
    assert gpu_rows(gpu_device, rec[:0], n[:0]) == []
    # argument errors in the stated order, with real memory behind every pointer
    rec_d, n_d = on(gpu_device, rec, n)
    lib, stream = E.load_library(), torch.cuda.current_stream().cuda_stream
    outs = [torch.zeros(3 * 384 + 4, dtype=torch.uint8, device=gpu_device), torch.zeros(3, dtype=torch.int32, device=gpu_device),
            torch.zeros(3, dtype=torch.uint8, device=gpu_device), torch.zeros(3, dtype=torch.int32, device=gpu_device),
            torch.zeros(3 * 29, dtype=torch.int32, device=gpu_device)]
    ptrs = [t.data_ptr() for t in outs]
    call = lambda rec=rec_d.data_ptr(), n=n_d.data_ptr(), P=3, budget=4096, ptrs=ptrs: lib.dsl_smiles_records(rec, n, P, budget, *ptrs, stream)
    assert call(budget=-1) == -1 and call(budget=E.GRAPH_MAX_NODES + 1) == -1 and call(P=-1) == -1 and call(P=2 ** 31) == -1
    assert call(P=0, rec=None, n=None, ptrs=[None] * 5) == 0
    assert call(rec=None) == -1 and call(n=None) == -1 and call(rec=rec_d.data_ptr() + 1248 + 2, P=1) == -1
    for k in range(5):
        assert call(ptrs=[None if j == k else x for j, x in enumerate(ptrs)]) == -1
    assert call(ptrs=[ptrs[0] + 1] + ptrs[1:]) == -1 and call(ptrs=[ptrs[0] + 4] + ptrs[1:]) == 0
    torch.cuda.synchronize()
    assert call() == 0
    torch.cuda.synchronize()
    assert outs[2].tolist() == [L.OVERFLOW, L.OK, L.OK]


# ------------------------------------------------------------------------------------------------------------------ the public interface

def test_exact_match_is_graph_identity_on_the_seeded_pairs(gpu_device, molecules):
    rec, n = molecules["rec"], molecules["n"]
    ref, prb = on(gpu_device, rec[molecules["ref"]], n[molecules["ref"]]), on(gpu_device, rec[molecules["prb"]], n[molecules["prb"]])
    match = S.smiles_exact_match(ref, prb)
    same = S.graph_identity_batch(ref, prb)
    assert isinstance(match, S.SmilesMatch) and match.same.dtype == torch.bool and match.same.device.type == gpu_device.type
    assert torch.equal(match.same, same.identical) and int(same.undecided.sum()) == 0 and int(match.status.sum()) == 0
    assert match.same.cpu().tolist() == GM.seeded_labels(2000).tolist()
    # with a row map, and from results computed before
    idx = torch.arange(1999, -1, -1, device=gpu_device)
    found_ref, found_prb = S.smiles(*ref), S.smiles(prb[0], prb[1].tolist())
    flipped = S.smiles_exact_match(found_ref, found_prb, ref_index=idx)
    assert torch.equal(flipped.same, S.graph_identity_batch(ref, prb, ref_index=idx).identical)
    strings = S.smiles_strings(found_ref)
    assert strings == [w["text"].decode() for w in molecules["want"][molecules["ref"]]] and isinstance(found_ref, S.Smiles)
    # the classes of graph_classes are the classes of the strings
    both = (torch.cat([ref[0], prb[0]])[::5].contiguous(), torch.cat([ref[1], prb[1]])[::5].contiguous())
    classes, texts = S.graph_classes(*both).cpu().tolist(), S.smiles_strings(S.smiles(*both))
    first = {}
    assert classes == [first.setdefault(t, p) for p, t in enumerate(texts)]


# ------------------------------------------------------------------------------------------------------------------ evaluation

def test_evaluate_reports_the_strings(gpu_device, tmp_path, monkeypatch):
    """diffspectra_evaluate(structure_metrics=True) on filler weights, 3 steps, K = 2: with ``cfg.eval.smiles`` the 'structure' dict holds the
    entry, equal to the mirror on the run's records (one slot's record is replaced by its ground truth under another atom order: the same
    string there), and the file is written; without the flag the dict is what it was."""
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
    assert "smiles" not in plain
    cfg.eval.smiles = True
    cfg.eval.smiles_path = str(tmp_path / "strings" / "smiles.tsv")
    torch.manual_seed(42)
    res = EV.diffspectra_evaluate(cfg, str(tmp_path), table, structure_metrics=True)[40]
    monkeypatch.setattr(shard, "gather_by_slot", gather)
    st = res["metrics"]["structure"]
    assert set(st) == set(plain) | {"smiles"}
    for key, a in plain.items():                                                # nothing else changes
        if isinstance(a, (int, float, type(None))):
            assert a == st[key] or (a != a and st[key] != st[key]), key
    assert set(st["graph"]) == set(plain["graph"]) and torch.equal(st["graph"]["verdict"], plain["graph"]["verdict"])
    sm = st["smiles"]
    assert set(sm) == {"generated", "ground_truth", "same", "status", "pair_status", "exact_match", "unique", "distinct", "certified", "uncertified",
                       "overflow", "unusable", "top_k"}
    gen_rec = kept[-1].cpu().numpy()
    gen_n = np.array([len(atom) for _, atom, _, _ in res["processed_mols"]], np.int32)
    want_gen, want_gt = L.write_table(gen_rec, gen_n), L.write_table(gt_rec, gt_n)
    text = lambda r: r["text"].decode() if r["status"] <= 1 else None
    assert sm["generated"] == [text(r) for r in want_gen] and sm["ground_truth"] == [text(want_gt[int(r)]) for r in slot_ds]
    assert sm["status"].cpu().tolist() == [r["status"] for r in want_gen]
    stated = [g["status"] == 0 and want_gt[int(r)]["status"] == 0 and g["text"] == want_gt[int(r)]["text"] for g, r in zip(want_gen, slot_ds)]
    assert sm["same"].cpu().tolist() == stated and stated[planted] and sm["generated"][planted] == sm["ground_truth"][planted]
    assert torch.equal(sm["same"], (st["graph"]["verdict"] == 1) & (sm["pair_status"] == 0))
    n_ok = sum(g["status"] == 0 and want_gt[int(r)]["status"] == 0 for g, r in zip(want_gen, slot_ds))
    certified = [g["text"] for g in want_gen if g["status"] == 0]
    assert sm["exact_match"] == (sum(stated) / n_ok if n_ok else None) and sm["certified"] == len(certified) and sm["distinct"] == len(set(certified))
    assert sm["unique"] == (len(set(certified)) / len(certified) if certified else None)
    assert (sm["uncertified"], sm["overflow"], sm["unusable"]) == tuple([r["status"] for r in want_gen].count(k) for k in (1, 2, 3))
    hits = [any(stated[t * K_:(t + 1) * K_]) for t in range(T)]
    assert sm["top_k"]["hit"].cpu().tolist() == hits and hits[1] and float(sm["top_k"]["acc_at_k"]) == sum(hits) / T
    lines = open(cfg.eval.smiles_path).read().split("\n")
    assert lines[-1] == "" and lines[:-1] == [f"{p}\t{g or ''}\t{t or ''}" for p, (g, t) in enumerate(zip(sm["generated"], sm["ground_truth"]))]
