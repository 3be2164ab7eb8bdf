"""GPU: ``dsp_read_smiles`` (csrc/ds_reader.hip) and what ``structure_metrics`` and ``text_metrics`` build on it against the plain-Python mirror of
tests/smiles_reader_mirror.py, which is written from include/diffspectra_reader.h and pinned by tests/test_smiles_reader_cpu.py.  Every output is
a byte or an integer and is compared exactly."""
import numpy as np
import pytest
import torch

from diffspectra_amd import engine as E, structure_metrics as S, text_metrics as T
from tests import graph_mirror as GM, smiles_mirror as L, smiles_reader_mirror as R, structure_mirror as SM
from tests.helpers import to_dev

pytestmark = pytest.mark.gpu

GUARD_ROWS = 3
WAVES = E.READER_WAVES
WIDTHS = ((1248, torch.uint8), (4, torch.int32), (1, torch.uint8), (4, torch.int32), (4, torch.int32), (4, torch.int32), (4, torch.int32),
          (116, torch.int32), (4, torch.int32))                    # bytes per row and the view of every output, in the header's order


def raw_call(dev, text, length, max_nodes=4096):
    """``dsp_read_smiles`` itself on outputs that stand between guard rows filled with a pattern; returns the status and the nine views."""
    P = text.shape[0]
    raws = [torch.full((P + 2 * GUARD_ROWS, width), 0x5A, dtype=torch.uint8, device=dev) for width, _ in WIDTHS]
    views = [raw[GUARD_ROWS:GUARD_ROWS + P].view(dtype) for raw, (_, dtype) in zip(raws, WIDTHS)]
    st = E.load_library().dsp_read_smiles(text.data_ptr(), text.shape[1], length.data_ptr(), P, max_nodes, *(v.data_ptr() for v in views),
                                          torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for raw in raws:
        assert bool((raw[:GUARD_ROWS] == 0x5A).all()) and bool((raw[GUARD_ROWS + P:] == 0x5A).all()), "a guard row was written"
    return st, views


def rows_of(out):
    """The nine tensors of a call as the mirror's list of row dicts."""
    rec, n, status, where, atoms, flags, aromatic, pos, nodes = (t.cpu().numpy().reshape(t.shape[0], -1) for t in out)
    n, status, where, atoms, flags, aromatic, nodes = (a.reshape(-1) for a in (n, status, where, atoms, flags, aromatic, nodes))
    return [dict(rec=rec[p].tobytes(), n=int(n[p]), status=int(status[p]), where=int(where[p]), string_atoms=int(atoms[p]), flags=int(flags[p]),
                 aromatic=int(aromatic[p]), atom_pos=pos[p].tolist(), nodes=int(nodes[p])) for p in range(len(n))]


def gpu_rows(dev, strings, max_nodes=4096, stride=R.TEXT_BYTES):
    text, length = R.pack(strings, stride)
    st, views = raw_call(dev, to_dev(dev, text, torch.uint8), to_dev(dev, length, torch.int32), max_nodes)
    assert st == 0
    return rows_of(views)


def same_rows(got, want, strings):
    assert len(got) == len(want)
    for p, (g, w) in enumerate(zip(got, want)):
        assert g == w, (p, strings[p], {k: (g[k], w[k]) for k in R.FIELDS if g[k] != w[k] and k != "rec"}, g["rec"] == w["rec"])


@pytest.fixture(scope="module")
def tables():
    """The strings of the hand table, the error table and the 29 / 30 atom pairs with the rows they must give: computed once, never changed."""
    strings = [t[0] for t in R.hand_table()] + [t[0] for t in R.error_table()] + [s for pair in R.limit_pairs() for s in pair]
    return strings, [R.read(s) for s in strings]


# ------------------------------------------------------------------------------------------------------------------ the kernel

def test_tables_against_the_mirror_and_the_hand_rows(gpu_device, tables):
    strings, want = tables
    got = gpu_rows(gpu_device, strings)
    same_rows(got, want, strings)
    same_rows(got[:len(R.hand_table())], R.hand_rows(), strings)
    for g, (text, status, where, atoms, nodes) in zip(got[len(R.hand_table()):], R.error_table()):
        assert (g["status"], g["where"], g["string_atoms"], g["nodes"]) == (status, where, atoms, nodes), text
    assert all(g["nodes"] < 4096 and g["status"] != R.UNDECIDED for g in got)               # the default budget decides every entry


@pytest.mark.parametrize("P", [1, WAVES - 1, WAVES, WAVES + 1])
def test_partial_workgroups(gpu_device, tables, P):
    strings, want = tables
    for at in (0, 39, len(R.hand_table()) + 17):
        same_rows(gpu_rows(gpu_device, strings[at:at + P]), want[at:at + P], strings[at:at + P])


def _padded(length):
    """A string of exactly ``length`` bytes that reads ok: a bracket atom whose isotope digits take up the slack, nested branches behind it."""
    if length <= 2:
        return "CC"[:length]
    tail = next(t for t in ("(=O)(N(C(F)))[O-]", "(N)O", "") if length - 3 - len(t) >= 0)
    return "[" + "9" * (length - 3 - len(tail)) + "C]" + tail


def test_seams(gpu_device):
    strings = [_padded(k) for k in (0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 383, 384)]
    strings += ["[" + "9" * 57 + "C][NH3+]",                         # a bracket atom over bytes 60..65
                "[" + "9" * 58 + "C]C%12CC%12",                      # a %nn over bytes 62..64
                "[" + "9" * 59 + "C]C%12CC%12", "[" + "9" * 57 + "C]C%12CC%12", "[" + "9" * 58 + "C](C)[C@@H](N)O", "[" + "9" * 59 + "C]=[N+]=[N-]",
                "[C](" * 28 + "[C]" + ")" * 28,                      # nesting depth 28, 29 atoms
                "[C](" * 29 + "[C]" + ")" * 29,
                "[C]0[C]9[C]%10[C]%99[C]0[C]9[C]%10[C]%99", "C0CCC9CCC%10CCC%99CCC0CC9CC%10CC%99", "C%00CC0",
                "[" + "9" * 380 + "C]", "C" * 384, "(" * 384, "C(" * 192, "[C]1" * 96, "C1" * 192, "C%12" * 96, "c1ccccc1" * 48]
    want = [R.read(s) for s in strings]
    assert [w["status"] for w in want[1:17]] == [R.OK] * 16 and want[0]["status"] == R.EMPTY and [len(s) for s in strings[:17]][-1] == 384
    assert want[23]["status"] == R.OK and want[23]["n"] == 29 and want[24]["status"] == R.TOO_LARGE and want[25]["status"] == R.OK
    same_rows(gpu_rows(gpu_device, strings), want, strings)
    for stride in (4, 64, 128):                                     # the same strings at short strides: too long where they do not fit
        short = [R.read(t.tobytes(), int(k), stride) for t, k in zip(*R.pack(strings, stride))]
        assert R.TOO_LONG in {w["status"] for w in short}
        same_rows(gpu_rows(gpu_device, strings, stride=stride), short, strings)


@pytest.fixture(scope="module")
def generated_rows():
    """2 000 generator strings and 2 000 single-byte edits of them with the mirror's rows: computed once, shared, never changed."""
    good, bad = list(R.generated(2000)), list(R.edited(2000))
    text, length = R.pack(bad, R.EDIT_STRIDE)
    return dict(good=good, want_good=[R.read(s) for s in good], bad=bad,
                want_bad=[R.read(text[k].tobytes(), int(length[k]), R.EDIT_STRIDE, R.EDIT_MAX_NODES) for k in range(len(bad))])


def test_generated_and_edited_rows(gpu_device, generated_rows):
    g = generated_rows
    assert all(w["status"] == R.OK for w in g["want_good"]) and {w["status"] for w in g["want_bad"]} == set(range(8))
    same_rows(gpu_rows(gpu_device, g["good"]), g["want_good"], g["good"])
    same_rows(gpu_rows(gpu_device, g["bad"], max_nodes=R.EDIT_MAX_NODES, stride=R.EDIT_STRIDE), g["want_bad"], g["bad"])


def test_max_nodes(gpu_device):
    naphthalene = "c1ccc2ccccc2c1"
    for budget in (0, 1, 4, 5):
        got, want = gpu_rows(gpu_device, [naphthalene, "CCO"], max_nodes=budget), [R.read(naphthalene, max_nodes=budget), R.read("CCO", max_nodes=budget)]
        same_rows(got, want, [naphthalene, "CCO"])
        assert got[0]["status"] == (R.OK if budget >= 5 else R.UNDECIDED) and got[0]["nodes"] == min(budget, 5) and got[1]["status"] == R.OK
    assert got[0]["n"] == 18


def test_repeat_runs_and_row_order(gpu_device, generated_rows):
    strings = generated_rows["good"][:300] + generated_rows["bad"][:300]
    text, length = (to_dev(gpu_device, a, dt) for a, dt in zip(R.pack(strings), (torch.uint8, torch.int32)))
    one, two = E.read_smiles(text, length), E.read_smiles(text, length)
    assert all(torch.equal(a, b) for a, b in zip(one, two))
    perm = torch.randperm(len(strings), generator=torch.Generator().manual_seed(5)).to(gpu_device)
    moved = E.read_smiles(text[perm].contiguous(), length[perm].contiguous())
    assert all(torch.equal(m, a[perm]) for m, a in zip(moved, one))
    st, views = raw_call(gpu_device, text, length)
    assert st == 0 and all(torch.equal(v.reshape(a.shape), a) for v, a in zip(views, one))
    empty = E.read_smiles(text[:0], length[:0])
    assert [tuple(t.shape) for t in empty] == [(0, 1248), (0,), (0,), (0,), (0,), (0,), (0,), (0, 29), (0,)]


def test_argument_errors(gpu_device):
    text, length = (to_dev(gpu_device, a, dt) for a, dt in zip(R.pack(["CCO", "c1ccccc1"]), (torch.uint8, torch.int32)))
    lib, stream = E.load_library(), torch.cuda.current_stream().cuda_stream
    out = [torch.zeros(2, width, dtype=torch.uint8, device=gpu_device) for width, _ in WIDTHS]
    ptrs = [t.data_ptr() for t in out]
    call = lambda text_p=text.data_ptr(), stride=384, len_p=length.data_ptr(), P=2, budget=4096, outs=ptrs: \
        lib.dsp_read_smiles(text_p, stride, len_p, P, budget, *outs, stream)
    assert call() == 0
    # in the header's order: the scalars first, also with P = 0 ...
    assert call(budget=-1) == -1 and call(budget=E.GRAPH_MAX_NODES + 1) == -1 and call(budget=E.GRAPH_MAX_NODES) == 0
    assert call(P=-1) == -1 and call(P=1 << 31) == -1
    assert [call(stride=s) for s in (0, 2, 6, 388, -4)] == [-1] * 5 and call(stride=6, P=0) == -1 and call(budget=-1, P=0) == -1
    # ... then P = 0 returns at once, whatever the pointers
    assert lib.dsp_read_smiles(0, 4, 0, 0, 0, *([0] * 9), stream) == 0
    # ... then the inputs, the outputs, the alignment of rec
    assert call(text_p=0) == -1 and call(len_p=0) == -1 and call(text_p=text.data_ptr() + 1) == -1
    for k in range(9):
        assert call(outs=ptrs[:k] + [0] + ptrs[k + 1:]) == -1, k
    assert call(outs=[ptrs[0] + 2] + ptrs[1:]) == -1
    torch.cuda.synchronize()
    # the binding
    with pytest.raises(TypeError):
        E.read_smiles(text.to(torch.int32), length)
    with pytest.raises(TypeError):
        E.read_smiles(text, length.to(torch.int64))
    with pytest.raises(ValueError):
        E.read_smiles(text[:, :6].contiguous(), length)
    with pytest.raises(ValueError):
        E.read_smiles(text, length[:1])
    with pytest.raises(ValueError):
        E.read_smiles(text, length, max_nodes=-1)
    with pytest.raises(TypeError):
        E.read_smiles(text, length, max_nodes=1.5)
    with pytest.raises(RuntimeError):
        E.read_smiles(text.cpu(), length.cpu())


# ------------------------------------------------------------------------------------------------------------------ round trip on the device

def test_round_trip_with_the_writer_on_the_device(gpu_device):
    ref, _, _ = GM.seeded_pairs(2000)
    want = L.seeded_rows(2000)[0]
    rec, n = SM.records(list(ref))
    rec, n = to_dev(gpu_device, rec, torch.uint8), to_dev(gpu_device, n, torch.int32)
    written = S.smiles(rec, n)
    back = S.read_smiles(written)                                    # the text / length tensors as they stand
    status = written.status.cpu()
    assert status.tolist() == [w["status"] for w in want] and int((status <= 1).sum()) >= 1990
    has_text = (status <= 1).to(gpu_device)
    assert bool((back.status[has_text] == 0).all()) and bool((back.n_atoms[has_text] == n[has_text]).all())
    assert bool((back.flags[has_text] == 0).all()) and bool((back.nodes == 0).all())
    same = S.graph_identity_batch((rec, n), (back.records, back.n_atoms))
    assert bool((same.verdict[has_text] == E.GRAPH_IDENTICAL).all())
    again = S.smiles(back.records, back.n_atoms)
    ok = (status == 0).to(gpu_device)
    assert bool((again.text[ok] == written.text[ok]).all()) and bool((again.status[ok] == 0).all())
    # strings, a Smiles result and tensors are one input
    strings = S.smiles_strings(written)[:50]
    from_strings = S.read_smiles(strings, device=gpu_device)
    assert all(torch.equal(a, b[:50]) for a, b in zip(from_strings, back))
    table, count = S.records_from_smiles(strings + ["C(", "CS"], device=gpu_device)
    assert torch.equal(table, back.records[:50]) and torch.equal(count, back.n_atoms[:50])


# ------------------------------------------------------------------------------------------------------------------ the metric table

PAIRS = (("OCC", "C(O)C"), ("C-C-O", "[CH3][CH2][OH]"), ("C1.O1C", "OCC"), ("C%10%11.C%10.C%11", "C(C)(C)C"), ("c1ccccc1", "C1=CC=CC=C1"),
         ("c1ccncc1", "c1ccccc1"), ("c1cc[nH]c1", "[nH]1cccc1"), ("c1ccoc1", "c1cc[nH]c1"), ("O=c1cccc[nH]1", "c1ccccc1O"),
         ("c1ccc2ccccc2c1", "c1ccc2cccc2cc1"), ("c1ccccc1c1ccccc1", "c1ccc(cc1)-c1ccccc1"), ("Cc1ccccn1", "n1ccccc1C"),
         ("C[N+](=O)[O-]", "CN(=O)=O"), ("[NH3+]CC(=O)[O-]", "N(C)(C)C"), ("N#N", "O=C=O"), ("C#N", "C#N"), ("C=1CCCCC=1", "C=1CCCCC1"),
         ("C12CC1C2", "C1CC1C1CC1"), ("F/C=C/F", "C\\C=C\\C"), ("C[C@H](N)O", "C[C@@H](N)O"), ("c1cnc[nH]1", "c1cc[nH]c1"),
         ("[O-][n+]1ccccc1", "c1ccncc1"), ("C.C", "C:C"), ("CS", "C"))


def _record_level(dev, ref, prb):
    """The seven numbers and the exact-match rate from the record-level calls on two record tables, over the pairs whose records both pass the
    valence check; also that mask."""
    valid = S.valence_batch(ref[0], ref[1]).valid & S.valence_batch(prb[0], prb[1]).valid
    keep = valid.nonzero().reshape(-1)
    ref, prb = tuple(t[keep].contiguous() for t in ref), tuple(t[keep].contiguous() for t in prb)
    mean = lambda v, k: float(v.double()[k].mean())
    mces, morgan = S.mces_batch(ref, prb), S.morgan_similarity_batch(ref, prb)
    maccs, fraggle = S.maccs_similarity_batch(prb[0], prb[1], ref[0], ref[1]), S.fraggle_similarity_batch(prb[0], prb[1], ref[0], ref[1])
    groups = S.functional_group_similarity_batch(ref, prb)
    every = torch.ones_like(keep, dtype=torch.bool)
    numbers = {"Top-1 Accuracy": mean(S.mobile_identity_batch(ref, prb).identical, every), "MCES": mean(mces.dist, mces.status != 3),
               "Tanimoto Similarity (Morgan)": mean(morgan.tanimoto, morgan.valid), "Cosine Similarity (Morgan)": mean(morgan.cosine, morgan.valid),
               "Tanimoto Similarity (MACCS)": mean(maccs.tanimoto, maccs.valid), "Fraggle Similarity": mean(fraggle.fraggle, fraggle.valid),
               "Functional Group Similarity": mean(groups.similarity, groups.valid),
               "smiles_exact_match": mean(S.smiles_exact_match(ref, prb).same, every)}
    return numbers, valid.cpu().tolist()


def test_evaluate_smiles_pairs_against_the_record_level_calls(gpu_device):
    assert len(PAIRS) == 24
    by_text = {t[0]: R.hand_record(t[1], t[2], t[3], t[4]) for t in R.hand_table()}
    hand = lambda texts: (to_dev(gpu_device, np.stack([np.frombuffer(by_text[s][0], np.uint8) for s in texts]), torch.uint8),
                          to_dev(gpu_device, np.array([by_text[s][1] for s in texts]), torch.int32))
    want, valid = _record_level(gpu_device, hand([t for _, t in PAIRS[:23]]), hand([p for p, _ in PAIRS[:23]]))
    got = T.evaluate_smiles_pairs([p for p, _ in PAIRS], [t for _, t in PAIRS], device=gpu_device)
    assert got["pairs"] == 24 and got["converted"] == sum(valid) >= 18 and got["converted_mask"] == valid + [False]
    assert got["invalid"] == dict(total=24 - sum(valid), valence=23 - sum(valid), predicted={"element": 1}, true={})
    for name, value in want.items():
        print(name, got[name], value)
        assert got[name] == value, name
    assert got["Top-1 Accuracy"] > 0.3 and all(len(v) == sum(valid) for v in got["detailed"].values())      # nine pairs are one molecule twice
    nothing = T.evaluate_smiles_pairs(["C(", "CS"], ["C", ""], device=gpu_device)
    assert nothing["converted"] == 0 and nothing["MCES"] is None and nothing["invalid"]["predicted"] == {"syntax": 1, "element": 1}
    assert nothing["invalid"]["true"] == {"empty": 1}


def test_tsv_end_to_end(gpu_device, tmp_path):
    """Original records -> strings -> the file of ``config.eval.smiles_path`` -> the metric table: the numbers of the record-level calls on the
    original records, although reading renumbers the atoms."""
    rng = np.random.default_rng(20261024)
    small = [w for w in (R.read(s) for s in R.generated(2000)[:600]) if 4 <= w["n"] <= 18][:121]
    mols = [GM.permuted(R.molecule(w), rng) for w in small]
    ref = mols[:120]
    prb = [GM.permuted(m, rng) if k % 3 == 0 else mols[k + 1] for k, m in enumerate(ref)]
    on = lambda ms: tuple(to_dev(gpu_device, a, dt) for a, dt in zip(SM.records(ms), (torch.uint8, torch.int32)))
    ref_t, prb_t = on(ref), on(prb)
    texts = [S.smiles_strings(S.smiles(*t)) for t in (prb_t, ref_t)]
    assert all(s is not None for side in texts for s in side)
    path = tmp_path / "smiles.tsv"
    path.write_text("".join(f"{k}\t{g}\t{t}\n" for k, (g, t) in enumerate(zip(*texts))))
    want, valid = _record_level(gpu_device, ref_t, prb_t)
    got = T.evaluate_jsonl_predictions(str(path), str(tmp_path / "table.csv"))
    assert got["pairs"] == 120 and got["converted_mask"] == valid and sum(valid) >= 30 and got["invalid"]["predicted"] == {} == got["invalid"]["true"]
    for name, value in want.items():
        print(name, got[name], value)
        assert got[name] == value, name
    assert 0.2 <= got["Top-1 Accuracy"] < 1.0                         # every third pair is one molecule twice
    lines = (tmp_path / "table.csv").read_text(encoding="utf-8-sig").splitlines()
    assert lines[0] == "Evaluation Metric,Value" and lines[1] == f"Top-1 Accuracy,{want['Top-1 Accuracy']:.4f}" and len(lines) == 8
    assert (tmp_path / "table_detailed_scores.csv").exists() and (tmp_path / "table_detailed_scores.json").exists()
    # the same pairs as lists and as JSONL
    as_lists = T.evaluate_jsonl_predictions((texts[1], texts[0]))
    jsonl = tmp_path / "pairs.jsonl"
    import json
    jsonl.write_text("".join(json.dumps({"predict": T.PREFIX + g, "label": T.PREFIX + t}) + "\n" for g, t in zip(*texts)))
    as_jsonl = T.evaluate_jsonl_predictions(str(jsonl))
    assert all(as_lists[name] == got[name] == as_jsonl[name] for name in T.METRIC_NAMES)
