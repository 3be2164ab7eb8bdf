"""CPU: the structure metric's C-ABI surface, its argument checks, the CPU mirror against cases whose answer is known by construction,
ground-truth records from a processed file, and the Top-K reductions.  (The kernel itself is checked on the GPU against the same mirror:
tests/test_structure_metrics_gpu.py.)"""
import re

import numpy as np
import pytest
import torch

from diffspectra_amd import engine as E, filler, shard
from tests import structure_mirror as SM


def test_header_declares_and_library_exports_match_records():
    import __graft_entry__ as g
    g.build()
    assert "ds_match_records" in E.EXPORTS and E.CONSTS["DS_RECORD_BYTES"] == shard.RECORD_BYTES == SM.RECORD_BYTES
    lib = E.load_library()
    assert hasattr(lib, "ds_match_records")
    hdr = re.sub(r"/\*.*?\*/", "", open(E.HEADER_PATH).read(), flags=re.S)
    args = re.search(r"int\s+ds_match_records\s*\((.*?)\)\s*;", hdr, flags=re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == [
        "prb_rec", "prb_n", "P", "ref_rec", "ref_n", "M", "ref_index", "max_distance", "min_atoms", "rmsd", "n_matched", "type_acc", "bond_acc",
        "exact", "map", "stream"]


def test_match_records_refuses_wrong_arguments():
    """Arguments are checked, never converted; and there is no CPU path."""
    rec = torch.zeros(4, shard.RECORD_BYTES, dtype=torch.uint8)
    n = torch.full((4,), 3, dtype=torch.int32)
    idx = torch.zeros(4, dtype=torch.int64)
    for fn in (E.match_records, E.DmtEngine.match_records.__get__(object())):
        with pytest.raises(TypeError, match="prb_rec"):
            fn(rec.float(), n, rec, n)
        with pytest.raises(TypeError, match="prb_n"):
            fn(rec, n.long(), rec, n)
        with pytest.raises(TypeError, match="ref_n"):
            fn(rec, n, rec, n.long())
        with pytest.raises(TypeError, match="ref_index"):
            fn(rec, n, rec, n, idx.int())
        with pytest.raises(ValueError, match="ref_rec"):
            fn(rec, n, rec[:, :1247].contiguous(), n)
        with pytest.raises(ValueError, match="prb_n"):
            fn(rec, n[:3], rec, n)
        with pytest.raises(ValueError, match="ref_index"):
            fn(rec, n, rec, n, idx[:2])
        with pytest.raises(ValueError, match="contiguous"):
            fn(torch.zeros(shard.RECORD_BYTES, 4, dtype=torch.uint8).t(), n, rec, n)
        with pytest.raises(ValueError, match="rows"):
            fn(rec, n, rec[:2], n[:2])                       # identity pairing needs a row per pair
        with pytest.raises(ValueError, match="NaN"):
            fn(rec, n, rec, n, None, float("nan"))
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(rec, n, rec, n, idx)
    from diffspectra_amd.structure_metrics import hungarian_rmsd_batch
    with pytest.raises(RuntimeError, match="no CPU path"):
        hungarian_rmsd_batch((rec, n), (rec, n))


# ------------------------------------------------------------------------------------------------------------------ mirror, known answers

def _molecule(n=9, seed=5):
    rng = np.random.default_rng(seed)
    pos, _, _, bond = SM.random_tree_molecule(rng, n)
    types = np.array(([1, 1, 3] + [0] * 26)[:n])             # C C O H...
    return dict(pos=pos.astype(np.float32).astype(np.float64), type=types, fc=np.zeros(n, np.int64), bond=bond), rng


def _small_rotation(degrees=5.0):
    """Rodrigues rotation about (1, 2, 3).  The reference's procedure is NOT rotation invariant: its first match runs on the unrotated
    centred coordinates (rmsd.py:45-48), so a large rotation scrambles it and the Kabsch fit with it.  At 5 degrees every atom of these
    molecules (radius < 5 A) moves less than 0.45 A, half the 0.9 A exclusion radius of the generator: each atom's own image is then its
    nearest ground-truth atom, the identity is the term-by-term minimum of the first match, and the expected map follows by hand."""
    k = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    t = np.deg2rad(degrees)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


def _moved(mol, rng, perm):
    """mol rotated, shifted and permuted: candidate atom i is atom perm[i] of mol."""
    assert np.sqrt(((mol["pos"] - mol["pos"].mean(0)) ** 2).sum(1)).max() < 5.0
    pos = mol["pos"] @ _small_rotation() + np.array([[1.5, -2.0, 0.7]])
    return dict(pos=pos[perm], type=mol["type"][perm].copy(), fc=mol["fc"][perm].copy(), bond=mol["bond"][np.ix_(perm, perm)].copy())


def test_mirror_rotated_translated_permuted_copy():
    ref, rng = _molecule()
    perm = rng.permutation(9)
    out = SM.match_pair(_moved(ref, rng, perm), ref)
    assert out["valid"] and out["map"][:9].tolist() == perm.tolist() and (out["map"][9:] == -1).all()
    assert out["rmsd"] < 1e-6 and out["exact"] == 1 and out["n_matched"] == 9 and out["type_acc"] == 1 and out["bond_acc"] == 1


def test_mirror_one_type_changed():
    ref, rng = _molecule()
    perm = rng.permutation(9)
    prb = _moved(ref, rng, perm)
    prb["type"][int(np.where(perm == 0)[0][0])] = 2          # atom 0 of the ground truth is a C: the candidate says N
    out = SM.match_pair(prb, ref)
    assert out["map"][:9].tolist() == perm.tolist() and out["exact"] == 0 and out["rmsd"] < 1e-6
    assert out["type_acc"] == np.float32(8 / 9) and out["bond_acc"] == 1
    prb["type"][:] = ref["type"][perm]
    prb["fc"][3] = 1                                          # a formal charge alone also breaks exactness
    assert SM.match_pair(prb, ref)["exact"] == 0
    prb["fc"][3] = 0
    a, b = np.argwhere(np.triu(prb["bond"]) > 0)[0]
    prb["bond"][a, b] = prb["bond"][b, a] = prb["bond"][a, b] % 3 + 1     # ... and so does one bond order
    out = SM.match_pair(prb, ref)
    assert out["exact"] == 0 and out["type_acc"] == 1 and out["bond_acc"] == np.float32(35 / 36)


def test_mirror_far_atom_stays_unmapped():
    ref, rng = _molecule(15)
    perm = rng.permutation(15)
    prb = _moved(ref, rng, perm)
    prb["pos"][4] += np.array([8.0, 0.0, 0.0])
    out = SM.match_pair(prb, ref)
    assert out["valid"] and out["map"][4] == -1 and out["n_matched"] <= 14 and out["exact"] == 0
    loose = SM.match_pair(prb, ref, max_distance=np.inf)      # without clipping every atom is kept
    assert loose["n_matched"] == 15 and loose["map"][4] >= 0


def test_mirror_fewer_than_three_atoms_is_invalid():
    ref, rng = _molecule(9)
    two = dict(pos=ref["pos"][:2], type=ref["type"][:2], fc=ref["fc"][:2], bond=np.array([[0, 1], [1, 0]]))
    for prb, gt in ((two, ref), (ref, two), (two, two)):
        out = SM.match_pair(prb, gt)
        assert not out["valid"] and np.isnan(out["rmsd"]) and out["n_matched"] == 0 and (out["map"] == -1).all() and out["exact"] == 0
    assert SM.match_pair(two, two, min_atoms=2)["valid"]
    lone = dict(ref, bond=np.zeros((9, 9), np.int64))         # no bonds at all: the fragment is one atom
    assert SM.largest_fragment(lone) == [0] and not SM.match_pair(lone, ref)["valid"]


def test_mirror_equal_fragments_the_one_with_atom_0_wins():
    tri, rng = _molecule(3)
    other = tri["pos"] @ SM._rotation(rng) + 6.0
    pos = np.zeros((6, 3))
    pos[[0, 2, 4]], pos[[1, 3, 5]] = tri["pos"], other
    bond = np.zeros((6, 6), np.int64)
    for half in ([0, 2, 4], [1, 3, 5]):
        bond[np.ix_(half, half)] = tri["bond"]
    both = dict(pos=pos, type=np.array([1, 0, 1, 0, 3, 0]), fc=np.zeros(6, np.int64), bond=bond)
    assert SM.largest_fragment(both) == [0, 2, 4]
    out = SM.match_pair(both, tri)
    assert out["valid"] and out["map"][:6].tolist() == [0, -1, 1, -1, 2, -1] and out["rmsd"] < 1e-6 and out["exact"] == 0
    small_first = np.zeros((5, 5), np.int64)                  # a strictly larger fragment wins wherever it sits
    small_first[0, 1] = small_first[1, 0] = small_first[2, 3] = small_first[3, 2] = small_first[3, 4] = small_first[4, 3] = 1
    assert SM.largest_fragment(dict(type=np.zeros(5, np.int64), bond=small_first)) == [2, 3, 4]


def test_mirror_non_finite_coordinate_is_invalid():
    ref, rng = _molecule(9)
    for bad in (np.nan, np.inf):
        prb = _moved(ref, rng, np.arange(9))
        prb["pos"][2, 0] = bad
        for a, b in ((prb, ref), (ref, prb)):
            out = SM.match_pair(a, b)
            assert not out["valid"] and out["n_matched"] == 0 and (out["map"] == -1).all()


def test_record_round_trip():
    ref, _ = _molecule(7)
    rec = SM.record_from_mol(ref["pos"], ref["type"], ref["fc"] - 1, ref["bond"])
    back = SM.mol_from_record(rec, 7)
    assert np.array_equal(back["pos"], ref["pos"]) and np.array_equal(back["type"], ref["type"]) and (back["fc"] == -1).all()
    assert np.array_equal(back["bond"], ref["bond"])


# ------------------------------------------------------------------------------------------------------------------ ground truth records

def _graph_molecules(count, seed=11):
    rng = np.random.default_rng(seed)
    mols = []
    for i in range(count):
        n = int(rng.integers(3, 12))
        pos, types, fc, bond = SM.random_tree_molecule(rng, n)
        if i == 1:
            a, b = np.argwhere(np.triu(bond) > 0)[0]
            bond[a, b] = bond[b, a] = 4                       # an aromatic code: no bond in the dense matrix (build_dataset.py:118-119)
        src, dst = np.nonzero(bond)
        mols.append({"atom_type": torch.tensor(types), "pos": torch.tensor(pos, dtype=torch.float32), "fc": torch.tensor(fc),
                     "edge_index": torch.tensor(np.stack([src, dst])), "edge_type": torch.tensor(bond[src, dst]),
                     "uv": filler.uniform(f"sm.uv{i}", (1, 701)).abs(), "ir": filler.uniform(f"sm.ir{i}", (1, 3501)).abs(),
                     "raman": filler.uniform(f"sm.ra{i}", (1, 3501)).abs()})
    return mols


def _expected_records(mols, ids):
    rows = []
    for j in ids:
        m = mols[j]
        n = m["atom_type"].numel()
        dense = torch.zeros(n, n, dtype=torch.int64)
        et = m["edge_type"].clone()
        et[et == 4] = 0
        dense[m["edge_index"][0], m["edge_index"][1]] = et
        rows.append(shard.pack_records_u8(m["pos"][None], m["atom_type"][None], m["fc"][None], dense[None]))
    return torch.cat(rows)


@pytest.mark.parametrize("layout", ["pyg2", "pyg1"])
def test_gt_records_from_processed_file(tmp_path, layout):
    from types import SimpleNamespace
    from diffspectra_amd.dataset_pack import PackedSpectraTable
    from diffspectra_amd.qm9s_reader import ProcessedQM9S
    from tests.test_host_cpu import _write_processed_qm9s
    mols = _graph_molecules(10)
    perm = _write_processed_qm9s(str(tmp_path / "processed"), mols, layout)
    ds = ProcessedQM9S(str(tmp_path))
    tab = ds.packed_table("ir", split="test")
    test_ids = perm[6:].tolist()
    assert tab.gt_records.dtype == torch.uint8 and tab.gt_records.shape == (len(test_ids), shard.RECORD_BYTES)
    assert torch.equal(tab.gt_records, _expected_records(mols, test_ids))
    every = ds.packed_table("ir", split=None)
    assert torch.equal(every.gt_records, _expected_records(mols, range(10)))
    assert every.num_atom.tolist() == [m["atom_type"].numel() for m in mols]
    # the same through items (the reference's dataset objects carry the graph fields)
    items = [SimpleNamespace(num_atom=torch.tensor(m["atom_type"].numel()), rdmol=None, **m) for m in mols]
    from_items = PackedSpectraTable.from_dataset(items, "ir")
    assert torch.equal(from_items.gt_records, every.gt_records)
    # a table built the old way carries none and behaves as before
    old = PackedSpectraTable([None, torch.cat([m["ir"] for m in mols]), None], every.num_atom, [m["pos"] for m in mols], None)
    assert old.gt_records is None and torch.equal(old.batch([3, 1], "ir")[0], torch.stack([mols[3]["ir"], mols[1]["ir"]]))
    no_fc = [SimpleNamespace(**{k: v for k, v in vars(it).items() if k != "fc"}) for it in items]      # one rule for both sources: all five fields
    assert PackedSpectraTable.from_dataset(no_fc, "ir").gt_records is None
    bare = PackedSpectraTable.from_dataset([SimpleNamespace(ir=m["ir"], num_atom=3, pos=m["pos"]) for m in mols], "ir")
    assert bare.gt_records is None
    with pytest.raises(ValueError, match="gt_records"):
        PackedSpectraTable([None, torch.cat([m["ir"] for m in mols]), None], every.num_atom, gt_records=every.gt_records[:3])
    # a file without formal charges holds no complete graph: no records
    for m in mols:
        del m["fc"]
    _write_processed_qm9s(str(tmp_path / "nofc" / "processed"), mols, layout)
    assert ProcessedQM9S(str(tmp_path / "nofc")).packed_table("ir", split="test").gt_records is None


def test_evaluate_refuses_structure_metrics_without_ground_truth(tmp_path):
    from diffspectra_amd import evaluate as EV
    from diffspectra_amd.config import qm9s_config
    with pytest.raises(ValueError, match="gt_records"):
        EV.diffspectra_evaluate(qm9s_config("ir"), str(tmp_path), [], structure_metrics=True)


# ------------------------------------------------------------------------------------------------------------------ Top-K

def test_topk_summary():
    from diffspectra_amd.structure_metrics import PairMetrics, topk_summary
    nan = float("nan")
    rmsd = torch.tensor([0.5, 0.2, nan,   nan, nan, nan,   nan, 1.5, 0.9,   0.0, 0.3, 0.1], dtype=torch.float64)
    exact = torch.tensor([0, 0, 0,   0, 0, 0,   0, 0, 0,   1, 0, 1], dtype=torch.uint8)
    z = torch.zeros(12)
    per_pair = PairMetrics(rmsd, z.int(), z, z, exact, torch.full((12, 29), -1, dtype=torch.int32))
    for arg in (per_pair, dict(rmsd=rmsd, exact=exact)):
        s = topk_summary(arg, 3)
        assert s["best_index"].tolist() == [1, -1, 2, 0] and s["hit"].tolist() == [False, False, False, True]
        assert torch.isnan(s["best_rmsd"][1]) and s["best_rmsd"][[0, 2, 3]].tolist() == [0.2, 0.9, 0.0]
        assert float(s["hit_at_k"]) == 0.25
    one = topk_summary(per_pair, 1)
    assert one["best_index"].tolist() == [0, 0, -1, -1, -1, -1, -1, 0, 0, 0, 0, 0] and float(one["hit_at_k"]) == 2 / 12
    assert per_pair.valid.tolist() == (~torch.isnan(rmsd)).tolist()
    with pytest.raises(ValueError):
        topk_summary(per_pair, 5)
