"""CPU: the plain-Python mirror of ``dsp_read_smiles`` (tests/smiles_reader_mirror.py) against its hand tables, the generator's promise, the
round trip with the writer's mirror, the Kekule search against a brute-force enumeration, and the host side of the text evaluation (packing,
loaders, CSV layout).  The kernel itself is compared with the mirror in tests/test_smiles_reader_gpu.py."""
import csv
import itertools
import json

import numpy as np
import pytest
import torch

from diffspectra_amd import abi, structure_metrics as S, text_metrics as T
from tests import graph_mirror as GM, smiles_mirror as L, smiles_reader_mirror as R


# ------------------------------------------------------------------------------------------------------------------ header and constants

def test_header_is_parsed_and_matches_the_mirror():
    c = abi.READER.consts
    assert [c["DSP_" + k] for k in ("OK", "EMPTY", "SYNTAX", "ELEMENT", "KEKULE", "TOO_LARGE", "UNDECIDED", "TOO_LONG")] == list(range(8))
    assert (R.OK, R.EMPTY, R.SYNTAX, R.ELEMENT, R.KEKULE, R.TOO_LARGE, R.UNDECIDED, R.TOO_LONG) == tuple(range(8))
    assert c["DSP_TEXT_BYTES"] == abi.SMILES.consts["DSL_TEXT_BYTES"] == R.TEXT_BYTES == 384
    assert [c["DSP_FLAG_" + k] for k in ("ISOTOPE", "CHIRAL", "DIRECTION", "CLASS", "AROMATIC")] == [1, 2, 4, 8, 16]
    assert abi.READER.exports("dsp_") == ["dsp_read_smiles"]
    proto = abi.READER.prototypes["dsp_read_smiles"]
    assert [t for _, t in proto.params] == ["*", "int32_t", "*", "int64_t", "int32_t"] + ["*"] * 10
    assert S.READER_STATUS_NAMES == R.STATUS_NAMES
    s = abi.SAMPLING.consts
    assert (R.TYPE, R.FC, R.BOND, R.RECORD_BYTES, R.W) == (s["DS_REC_TYPE"], s["DS_REC_FC"], s["DS_REC_BOND"], s["DS_RECORD_BYTES"], s["DS_MAX_ATOMS"])


def test_library_exports_the_reader():
    import __graft_entry__ as g
    from diffspectra_amd import engine as E
    g.build()
    assert hasattr(E.load_library(), "dsp_read_smiles")


# ------------------------------------------------------------------------------------------------------------------ the tables

def test_tables_are_as_large_as_promised():
    assert len(R.hand_table()) >= 40 and len(R.error_table()) >= 30
    assert len({t[0] for t in R.hand_table()}) == len(R.hand_table()) and len({t[0] for t in R.error_table()}) == len(R.error_table())


@pytest.mark.parametrize("k", range(len(R.hand_table())))
def test_hand_table(k):
    text = R.hand_table()[k][0]
    got, want = R.read(text), R.hand_rows()[k]
    assert got == want, (text, {f: (got[f], want[f]) for f in R.FIELDS if got[f] != want[f] and f != "rec"})
    mol = R.molecule(got)
    assert (np.asarray(mol["bond"]) == np.asarray(mol["bond"]).T).all() and not np.diag(mol["bond"]).any()


def test_error_table():
    for text, status, where, string_atoms, nodes in R.error_table():
        got = R.read(text)
        assert (got["status"], got["where"], got["string_atoms"], got["nodes"]) == (status, where, string_atoms, nodes), repr(text)
        assert got["n"] == 0 and got["rec"] == bytes(R.RECORD_BYTES) and got["aromatic"] == 0 and got["atom_pos"] == [-1] * R.W, repr(text)
        if status in (R.SYNTAX, R.ELEMENT, R.EMPTY):
            assert got["flags"] == 0


def test_limit_pairs_side_by_side():
    for small, large in R.limit_pairs():
        a, b = R.read(small), R.read(large)
        assert (a["status"], a["n"]) == (R.OK, 29) and (b["status"], b["n"], b["where"]) == (R.TOO_LARGE, 0, -1), (small, large)
        assert b["string_atoms"] > 0


def test_length_and_stride():
    assert R.read(b"CC", 2, stride=4)["status"] == R.OK
    assert R.read(b"CCCCC", 5, stride=4)["status"] == R.TOO_LONG and R.read(b"CC", -1)["status"] == R.TOO_LONG
    assert R.read(b"C" * 385, 385)["status"] == R.TOO_LONG and R.read(b"", 0)["status"] == R.EMPTY
    assert R.read(b"CC(", 2)["status"] == R.OK                       # bytes behind the length are not read


def test_max_nodes():
    naphthalene = "c1ccc2ccccc2c1"
    got = R.read(naphthalene, max_nodes=1)
    assert (got["status"], got["nodes"], got["where"], got["n"], got["string_atoms"]) == (R.UNDECIDED, 1, -1, 0, 10)
    assert R.read(naphthalene, max_nodes=5)["status"] == R.OK and R.read(naphthalene, max_nodes=4)["status"] == R.UNDECIDED
    assert R.read("CCO", max_nodes=0)["status"] == R.OK


# ------------------------------------------------------------------------------------------------------------------ the generator

def test_every_generated_row_reads_ok():
    rows = R.generated(2000)
    assert len(rows) == 2000 and len(set(rows)) > 1500
    got = [R.read(s) for s in rows]
    assert all(g["status"] == R.OK for g in got)
    assert max(g["n"] for g in got) == 29 and min(g["n"] for g in got) <= 3
    flags = 0
    for g in got:
        flags |= g["flags"]
    assert flags == 31
    assert sum(1 for s in rows if "%" in s) > 100 and sum(1 for s in rows if "." in s) > 100 and sum(1 for g in got if g["nodes"] > 3) > 100


def test_edited_rows_show_every_status():
    text, length = R.pack(R.edited(2000), R.EDIT_STRIDE)
    got = [R.read(text[k].tobytes(), int(length[k]), R.EDIT_STRIDE, R.EDIT_MAX_NODES) for k in range(2000)]
    assert {g["status"] for g in got} == set(range(8))


# ------------------------------------------------------------------------------------------------------------------ round trip with the writer

def _same_after_round_trip(mol):
    row = L.write(mol)
    if row["status"] not in (L.OK, L.UNCERTIFIED):
        return None
    got = R.read(row["text"])
    assert got["status"] == R.OK and got["flags"] == 0 and got["nodes"] == 0, row["text"]
    return GM.same_graph(R.molecule(got), mol)


def test_round_trip_of_the_property_molecules():
    answers = [_same_after_round_trip(m) for _, m in L.property_molecules()]
    assert answers.count(None) == 1 and all(a for a in answers if a is not None)        # k29 overflows the writer


def test_round_trip_of_seeded_rows():
    ref, prb, _ = GM.seeded_pairs(2000)
    ref_rows, prb_rows = L.seeded_rows(2000)
    for mol, row in list(zip(ref, ref_rows))[:150] + list(zip(prb, prb_rows))[:150]:
        got = R.read(row["text"])
        assert got["status"] == R.OK and GM.same_graph(R.molecule(got), mol), row["text"]
        assert got["string_atoms"] == L.parse(row["text"].decode())["string_atoms"]


# ------------------------------------------------------------------------------------------------------------------ the Kekule search

def _wanting_graph(text):
    """(wants, nb) of a string, through the mirror's own scan and ring test"""
    atoms, bonds, _ = R._scan(text.encode())
    S_ = len(atoms)
    nbr = [[] for _ in range(S_)]
    for a, b, _ in bonds:
        nbr[a].append(b)
        nbr[b].append(a)
    order = [[0] * S_ for _ in range(S_)]
    for a, b, code in bonds:
        if code in (0, R.SOFT):
            code = "a" if atoms[a]["arom"] and atoms[b]["arom"] and R._ring_bond(nbr, a, b) else 1
        order[a][b] = order[b][a] = code
    wants, nb, _ = R.wanting_graph(atoms, order)
    return wants, nb


def _all_matchings(wants, nb):
    """Every perfect matching, as sorted tuples of pairs, by brute force over the partners of the lowest free atom - in lexicographic order of
    the partner choices, which is the order of the stated depth-first search."""
    if not wants:
        return [()]
    u, out = wants[0], []
    for v in sorted(nb[u]):
        if v in wants:
            rest = [w for w in wants if w not in (u, v)]
            out += [((u, v),) + m for m in _all_matchings(rest, nb)]
    return out


def test_kekule_search_against_brute_force():
    aromatic = [t[0] for t in R.hand_table() if t[5] & R.F_AROMATIC] + [t[0] for t in R.error_table() if t[1] == R.KEKULE] + \
        ["c1ccc2cc3ccccc3cc2c1", "c1cc2cccc3ccc4cccc1c4c32", "c1ccc2c(c1)[nH]c1ccccc12", "c1ccc2ncccc2c1", "c1cc2ccc1cc2", "c1ccc2cccc2c1"]
    assert len(aromatic) >= 20
    decided = {True: 0, False: 0}
    for text in aromatic:
        wants, nb = _wanting_graph(text)
        every = _all_matchings(wants, nb)
        # an independent existence check for the small ones: some set of |wants| / 2 aromatic bonds covers every wanting atom
        edges = sorted({(a, b) for a in wants for b in nb[a] if a < b})
        if len(edges) <= 16:
            half, odd = divmod(len(wants), 2)
            exists = not odd and any(sorted(x for e in pick for x in e) == sorted(wants) for pick in itertools.combinations(edges, half))
            assert exists == bool(every), text
        status, mate, nodes, fail = R.kekule_search(wants, nb, 1 << 20)
        assert (status == R.OK) == bool(every), text
        decided[bool(every)] += 1
        if every:
            assert tuple(sorted((a, b) for a, b in mate.items() if a < b)) == tuple(sorted(every[0])), text
        else:
            assert fail in wants
    assert decided[True] >= 18 and decided[False] >= 3


# ------------------------------------------------------------------------------------------------------------------ the host side

def test_host_packing():
    text, length = S.pack_smiles(["  CCO\n", "", "C" * 400, "CéC", "c1ccccc1"])
    assert text.dtype == torch.uint8 and tuple(text.shape) == (5, 384) and length.dtype == torch.int32
    assert length.tolist() == [3, 0, 400, 3, 8]
    assert bytes(text[0, :4].tolist()) == b"CCO\0" and not text[1].any() and bytes(text[2].tolist()) == b"C" * 384
    assert text[3, :3].tolist() == [67, 255, 67]
    mine, theirs = R.pack(["CCO", "", "C" * 400, "C\xffC", "c1ccccc1"])
    assert (text.numpy() == mine).all() and (length.numpy() == theirs).all()
    assert R.read(text[3].numpy().tobytes(), 3)["status"] == R.SYNTAX and R.read(text[2].numpy().tobytes(), 400)["status"] == R.TOO_LONG


def test_loaders(tmp_path):
    j = tmp_path / "pairs.jsonl"
    j.write_text(json.dumps({"predict": "##SMILES: CCO", "label": "##SMILES: OCC", "more": 1}) + "\n\n" +
                 json.dumps({"predict": "c1ccccc1", "label": "##SMILES: C1=CC=CC=C1"}) + "\n")
    assert T.load_smiles_from_jsonl(str(j)) == [("CCO", "OCC"), ("c1ccccc1", "C1=CC=CC=C1")]
    t = tmp_path / "run.tsv"
    t.write_text("0\tCCO\tOCC\n1\t\tC\n2\tN\t\n")
    assert T.load_smiles_from_tsv(str(t)) == [("CCO", "OCC"), ("", "C"), ("N", "")]
    assert T._pairs_of(str(j)) == (["CCO", "c1ccccc1"], ["OCC", "C1=CC=CC=C1"]) and T._pairs_of(str(t))[1] == ["OCC", "C", ""]
    assert T._pairs_of((["OCC", "C"], [["CCO", "CC"], "N"])) == (["CCO", "N"], ["OCC", "C"])
    bad = tmp_path / "bad.tsv"
    bad.write_text("0\tCCO\n")
    with pytest.raises(ValueError):
        T.load_smiles_from_tsv(str(bad))


def test_csv_layout(tmp_path):
    result = {name: 0.123456 * (k + 1) for k, name in enumerate(T.METRIC_NAMES)}
    result["detailed"] = {name: [True, False] if k == 0 else [0.5 * k, None] for k, name in enumerate(T.METRIC_NAMES)}
    out = tmp_path / "table.csv"
    paths = T.write_tables(result, str(out))
    assert [p.split("/")[-1] for p in paths] == ["table.csv", "table_detailed_scores.csv", "table_detailed_scores.json"]
    raw = out.read_bytes()
    assert raw.startswith(b"\xef\xbb\xbf")
    assert raw[3:].decode().splitlines() == ["Evaluation Metric,Value", "Top-1 Accuracy,0.1235", "MCES,0.2469", "Tanimoto Similarity (Morgan),0.3704",
                                             "Cosine Similarity (Morgan),0.4938", "Tanimoto Similarity (MACCS),0.6173", "Fraggle Similarity,0.7407",
                                             "Functional Group Similarity,0.8642"]
    with open(paths[1], encoding="utf-8-sig", newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == list(T.METRIC_NAMES) and rows[1] == ["True", "0.5", "1.0", "1.5", "2.0", "2.5", "3.0"] and rows[2] == ["False"] + [""] * 6
    with open(paths[2], encoding="utf-8") as f:
        assert json.load(f) == result["detailed"]
