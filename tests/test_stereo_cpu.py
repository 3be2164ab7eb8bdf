"""CPU: the definition of include/diffspectra_stereo.h as tests/stereo_mirror.py restates it - the hand table, the invariances, the soundness of the
twin rule by brute force, the condition on the seeded pair set that the GPU tests rely on - and the C-ABI surface of the new header."""
import numpy as np
import pytest

from diffspectra_amd import abi
from tests import stereo_mirror as K

HEADER = abi.STEREO                       # include/diffspectra_stereo.h: the definition that the mirror restates
TABLE = K.hand_table()


@pytest.mark.parametrize("row", TABLE, ids=[t[0] for t in TABLE])
def test_hand_table(row):
    name, a, b, counts, verdict = row
    got = K.compare(a, b)
    assert got["verdict"] == verdict, (name, got["verdict"], got["found"])
    assert counts is None or tuple(got["found"]) == counts, (name, got["found"])
    assert got["margin"] > 0.3                                            # nothing in the table sits near a threshold
    for kind in ("same", "mirror"):
        assert all(K.map_claim(a, b, m + [-1] * (K.W - len(m)), K.IDENTICAL if kind == "same" else K.MIRROR) for m in got["maps"][kind])


def test_hand_table_sites():
    sites = {name: K.compare(a, b)["sites"] for name, a, b, _, _ in TABLE}
    assert sites["methane"] == [0, 0, 0, 0] and sites["neopentane"] == [1, 0, 0, 0] and sites["cubane"] == [8, 0, 0, 0]
    assert sites["1,3-difluoroallene / mirror image"] == [0, 0, 0, 0]     # the stated deviation: no site at all
    assert sites["(Z)- / (E)-1,2-difluoroethene"] == [0, 1, 0, 0] and sites["acetaldoxime / other isomer"] == [0, 1, 0, 0]
    assert sites["flattened 1-fluoroethanol"] == [1, 0, 1, 0]
    V = np.array([s["V"] for s in K.perceive(K.cubane())["tetra"]])
    assert np.allclose(np.abs(V), 1 + np.sqrt(3), atol=1e-6) and (V > 0).sum() == 4
    assert (V > 0).tolist() == [False, True, False, True, True, False, True, False]      # half of each sign (which half: the atom numbering decides)
    ideal = K.perceive(K.methane().copy() | dict(type=np.array([1, 0, 2, 3, 4])))["tetra"][0]["V"]
    assert abs(abs(ideal) - 16 / (3 * np.sqrt(3))) < 1e-6
    masks, vol, status = K.site_masks(K.fluoroethanol())
    assert status == 0 and masks[0] == 1 and masks[1] == 1 and masks[3] == 0 and masks[6] == 0b11100 and not np.isnan(vol[0]) and np.isnan(vol[1:]).all()


def test_invariance_under_renumbering_and_rotation():
    """Every output but the map is unchanged when either side is moved rigidly and its atoms renumbered."""
    rng = np.random.default_rng(41)
    prb, ref, _ = K.seeded_pairs()
    pairs = [(a, b) for _, a, b, _, _ in TABLE] + list(zip(prb, ref))[::5]
    for a, b in pairs:
        base = K.compare(a, b)
        for x, y in ((K.renumbered(a, rng), b), (a, K.renumbered(b, rng)), (K.renumbered(a, rng), K.renumbered(b, rng))):
            moved = K.compare(x, y)
            if min(base["margin"], moved["margin"]) > 1e-6:               # (fp32 rounding of the moved coordinates moves |V| by ~1e-7)
                assert (moved["verdict"], moved["found"], moved["sites"]) == (base["verdict"], base["found"], base["sites"])


def test_reflection_exchanges_identical_and_mirror():
    seen = set()
    prb, ref, _ = K.seeded_pairs()
    for a, b in [(a, b) for _, a, b, _, _ in TABLE] + list(zip(prb, ref)):
        base, turned = K.compare(a, b), K.compare(a, K.reflected(b))
        assert turned["sites"] == base["sites"] and turned["found"][0] == base["found"][0]
        if base["verdict"] in (K.IDENTICAL, K.MIRROR):
            chiral = base["found"][1] == 0 or base["found"][2] == 0         # no phi of the other kind: the pair tells the two images apart
            if base["sites"][0] and chiral:
                assert turned["verdict"] == K.IDENTICAL + K.MIRROR - base["verdict"] and turned["found"][1:] == base["found"][:0:-1]
            else:
                assert turned["verdict"] == base["verdict"] and turned["found"] == base["found"]
            seen.add((base["verdict"], bool(base["sites"][0] and chiral)))
        else:
            assert turned["verdict"] == base["verdict"]
    assert seen == {(1, True), (1, False), (4, True)}


def test_swapping_two_neighbours_inverts_that_site():
    for mol in (K.fluoroethanol(), K.difluorobutane(False), K.cubane()):
        site = K.perceive(mol)["tetra"][0]
        other = K.perceive(K.neighbours_swapped(mol, site["nbrs"][0], site["nbrs"][2]))["tetra"][0]
        assert other["atom"] == site["atom"] and other["positive"] != site["positive"] and abs(other["V"] + site["V"]) < 1e-9
    fe = K.fluoroethanol()
    assert K.compare(K.neighbours_swapped(fe, 1, 5), fe)["verdict"] == K.MIRROR
    two = K.difluorobutane(False)
    site = K.perceive(two)["tetra"][0]
    assert K.compare(K.neighbours_swapped(two, site["nbrs"][1], site["nbrs"][2]), two)["verdict"] == K.STEREOISOMER      # one of two centres: the meso form


def test_the_twin_rule_loses_nothing():
    """Brute force over ALL isomorphisms (every ordinal 0) gives the verdict of the ordinal-respecting ones, and every isomorphism is an
    ordinal-respecting one followed by twin swaps: the counts differ by the product of the twin classes' factorials."""
    from math import factorial
    for name, a, b, _, verdict in TABLE:
        if len(a["type"]) > 12 or len(a["type"]) != len(b["type"]):
            continue
        pa, pb = K.perceive(a), K.perceive(b)
        zero = [0] * len(a["type"])
        every = list(K.isomorphisms(a, b, zero, zero))
        kept = list(K.isomorphisms(a, b, pa["ordinal"], pb["ordinal"]))
        classes = {}
        are_twins, _, twin = K.twins_of(a)
        for i in range(len(twin)):
            if twin[i]:
                classes.setdefault(min(j for j in range(len(twin)) if j == i or are_twins(i, j)), []).append(i)
        swaps = int(np.prod([factorial(len(c)) for c in classes.values()])) if classes else 1
        assert len(every) == len(kept) * swaps, name
        if verdict in (K.IDENTICAL, K.MIRROR, K.STEREOISOMER):
            kinds = lambda maps: sorted(set(K.kind_of(b, pa, pb, m) for m in maps))
            assert kinds(every) == kinds(kept), name


def test_thresholds():
    fe = K.fluoroethanol()
    V = abs(K.perceive(fe)["tetra"][0]["V"])
    assert K.compare(fe, fe, min_volume=V - 1e-9)["verdict"] == K.IDENTICAL and K.compare(fe, fe, min_volume=V + 1e-9)["verdict"] == K.UNASSIGNED
    z = K.difluoroethene(True)
    twisted = dict(z, pos=z["pos"].copy())
    twisted["pos"][4] = (1.3, 0.0, 1.1)                                   # one end turned by 90 degrees: c = 0
    twisted["pos"][5] = (1.3, 0.0, -1.1)
    assert K.compare(twisted, z)["verdict"] == K.UNASSIGNED and K.compare(twisted, z)["sites"] == [0, 1, 1, 0]
    assert K.compare(twisted, z, min_planarity=0.0)["verdict"] in (K.IDENTICAL, K.STEREOISOMER, K.UNASSIGNED)
    from diffspectra_amd import engine as E
    assert E._stereo_thresholds(None, None) == [0.5, 0.5] == [E.STEREO_MIN_VOLUME, E.STEREO_MIN_PLANARITY] and E._stereo_thresholds(1, 0) == [1.0, 0.0]
    for bad in ((float("nan"), None), (None, -0.5), (-1e-9, 0.5)):
        with pytest.raises(ValueError):
            E._stereo_thresholds(*bad)


def test_seeded_set_condition():
    """What the GPU parity test relies on: no |V| and no |c| of the seeded set lies within 1e-6 of its threshold (so an fp64 rounding
    difference cannot flip an assigned bit), and the set holds every verdict a finished search can give."""
    prb, ref, names = K.seeded_pairs()
    res = K.seeded_results()
    assert len(prb) == len(ref) == len(names) == len(res) == 3 * (12 * 8 + 5)
    assert {len(m["type"]) for m in ref} == set(range(1, 13)) | {29}
    margin = min(r["margin"] for r in res)
    print(f"[stereo] seeded set: {len(res)} pairs, smallest margin {margin:.3e}, verdicts {np.bincount([r['verdict'] for r in res], minlength=7).tolist()}")
    assert margin >= 1e-6
    assert {r["verdict"] for r in res} == {K.DIFFERENT, K.IDENTICAL, K.MIRROR, K.STEREOISOMER, K.UNASSIGNED}
    assert all(r["verdict"] in (K.IDENTICAL, K.UNASSIGNED) for r, n in zip(res, names) if n.endswith(("identity", "moved")))


def test_abi_surface():
    hdr = HEADER
    assert hdr.exports("dsc_") == list(hdr.prototypes) == ["dsc_stereo_identity_records", "dsc_stereo_sites"]
    for other in (abi.SAMPLING, abi.TRAINING, abi.SETS, abi.VALENCE, abi.GROUPS, abi.SCAFFOLD, abi.SMILES, abi.SUBSTRUCTURE, abi.TILES, abi.STEP):
        assert other.exports("dsc_") == [] and not any(k.startswith("DSC_") for k in other.consts)
    c = hdr.consts
    assert [c["DSC_" + k] for k in ("DIFFERENT", "IDENTICAL", "UNDECIDED", "INVALID", "MIRROR", "STEREOISOMER", "UNASSIGNED")] == list(range(7))
    g = abi.SAMPLING.consts
    assert [c["DSC_" + k] for k in ("DIFFERENT", "IDENTICAL", "UNDECIDED", "INVALID")] == [g["DS_GRAPH_" + k] for k in ("DIFFERENT", "IDENTICAL", "UNDECIDED", "INVALID")]
    assert hdr.reals == {"DSC_MIN_VOLUME": 0.5, "DSC_MIN_PLANARITY": 0.5} and c["DSC_OK"] == 0 and c["DSC_UNUSABLE"] == 3 and c["DSC_NUM_MASKS"] == 7
    assert [c["DSC_MASK_" + k] for k in ("TETRA_SITE", "TETRA_ASSIGNED", "TETRA_POSITIVE", "EZ_SITE", "EZ_ASSIGNED", "EZ_CIS", "TWIN")] == list(range(7))
    assert (K.DIFFERENT, K.IDENTICAL, K.UNDECIDED, K.INVALID, K.MIRROR, K.STEREOISOMER, K.UNASSIGNED) == tuple(range(7))
    assert (K.MIN_VOLUME, K.MIN_PLANARITY) == (hdr.reals["DSC_MIN_VOLUME"], hdr.reals["DSC_MIN_PLANARITY"])
    pairs = hdr.prototypes["dsc_stereo_identity_records"]
    assert pairs.ret == "int" and [n for n, _ in pairs.params] == ["prb_rec", "prb_n", "P", "ref_rec", "ref_n", "M", "ref_index", "max_nodes", "min_volume",
                                                                    "min_planarity", "exhaustive", "verdict", "nodes", "found", "sites", "map", "stream"]
    assert [t for _, t in pairs.params] == ["*", "*", "int64_t", "*", "*", "int64_t", "*", "int32_t", "double", "double", "int32_t", "*", "*", "*", "*", "*", "*"]
    graph = abi.SAMPLING.prototypes["ds_graph_identity_records"]
    assert pairs.params[:8] == graph.params[:8]                           # the "record pairs" contract, argument for argument
    one = hdr.prototypes["dsc_stereo_sites"]
    assert [n for n, _ in one.params] == ["rec", "n", "P", "min_volume", "min_planarity", "masks", "volume", "status", "stream"]
    assert [t for _, t in one.params] == ["*", "*", "int64_t", "double", "double", "*", "*", "*", "*"]
    assert len(abi.SAMPLING.exports("ds_")) == 31                         # the sampling header is untouched


def test_python_surface():
    from diffspectra_amd import engine as E, structure_metrics as M
    import inspect
    assert list(inspect.signature(M.stereo_identity_batch).parameters) == ["ref", "prb", "ref_index", "max_nodes", "min_volume", "min_planarity", "exhaustive", "engine"]
    sig = inspect.signature(M.stereo_identity_batch).parameters
    assert (sig["ref_index"].default, sig["max_nodes"].default, sig["min_volume"].default, sig["min_planarity"].default, sig["exhaustive"].default,
            sig["engine"].default) == (None, 4096, None, None, False, None)
    assert M.StereoIdentity._fields == ("verdict", "nodes", "found", "sites", "map")
    for prop in ("identical", "mirror", "stereoisomer", "unassigned", "undecided", "same_constitution"):
        assert isinstance(getattr(M.StereoIdentity, prop), property)
    import torch
    v = M.StereoIdentity(torch.arange(7, dtype=torch.uint8), None, None, None, None)
    assert v.same_constitution.tolist() == [False, True, False, False, True, True, True] and v.mirror.tolist()[4] and v.unassigned.tolist()[6]
    assert M.StereoSites._fields == ("tetra_site", "tetra_assigned", "tetra_positive", "ez_site", "ez_assigned", "ez_cis", "twin", "volume", "status")
    assert callable(M.stereo_sites) and callable(M.chirality) and M.Chirality._fields == ("chiral", "automorphisms")
    assert hasattr(E.DmtEngine, "stereo_identity_records") and hasattr(E.DmtEngine, "stereo_sites")
    assert (E.STEREO_MIRROR, E.STEREO_STEREOISOMER, E.STEREO_UNASSIGNED) == (4, 5, 6)
    rec = torch.zeros(2, E.RECORD_BYTES, dtype=torch.uint8)
    n = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(RuntimeError):                                     # no CPU path
        E.stereo_identity_records(rec, n, rec, n)
    with pytest.raises(TypeError):
        E.stereo_identity_records(rec, n, rec, n, exhaustive="yes")
    with pytest.raises(ValueError):
        E.stereo_identity_records(rec, n, rec, n, max_nodes=-1)
