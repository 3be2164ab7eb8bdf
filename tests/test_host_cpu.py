"""CPU: host logic and the C-ABI surface (no compute calls — there is no GPU here)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from diffspectra_amd import engine as E, filler
from diffspectra_amd.config import qm9s_config
from tests.helpers import procedural_state_dict


def test_library_exports_every_declared_symbol():
    import __graft_entry__ as g
    g.build()
    lib = E.load_library()                      # includes the struct-size self check
    hdr = open(E.HEADER_PATH).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = re.findall(r"^\s*(?:int|void)\s+(ds_\w+)\s*\(", hdr, flags=re.M)
    assert len(declared) >= 11
    for name in declared:
        assert hasattr(lib, name), name
    # the training C-ABI (include/diffspectra_train.h) lives in the same library
    from diffspectra_amd import train_engine as T
    train = T.train_exports()
    assert len(train) >= 30 and "dst_gemm" in train and "dst_adamw_ema" in train
    tl = T.load_train_library()
    for name in train:
        assert hasattr(tl, name), name


def _headers():
    from diffspectra_amd import abi
    return abi, (abi.SAMPLING, abi.TRAINING)


def test_prototypes_match_a_hand_written_table():
    """``abi.Header.prototypes`` against prototypes copied by hand from the two headers: a void return, a plain ``int``, a struct pointer, a
    pointer to pointers, mixed 32 / 64-bit integers with ``float`` and ``double*``, ``uint64_t`` / ``uint32_t``, a ``double`` by value among floats."""
    abi, (smp, trn) = _headers()
    P, i32, i64, u32, u64, f, d = "*", "int32_t", "int64_t", "uint32_t", "uint64_t", "float", "double"
    want = {
        "ds_struct_sizes": ("void", [("out", P)]),
        "ds_set_two_stream": ("int", [("on", "int")]),
        "ds_gemm": ("int", [("args", P), ("stream", P)]),
        "ds_fingerprint": ("int", [("ptrs", P), ("prefix", P), ("n", i32), ("out", P), ("stream", P)]),
        "ds_match_records": ("int", [("prb_rec", P), ("prb_n", P), ("P", i64), ("ref_rec", P), ("ref_n", P), ("M", i64), ("ref_index", P),
                                     ("max_distance", f), ("min_atoms", i32), ("rmsd", P), ("n_matched", P), ("type_acc", P), ("bond_acc", P),
                                     ("exact", P), ("map", P), ("stream", P)]),
        "ds_initial_noise": ("int", [("L", P), ("seed", u64), ("mol_id", P), ("x", P), ("edge_x", P), ("stream", P)]),
        "dst_adamw_ema": ("int", [("p", P), ("g", P), ("m", P), ("v", P), ("vmax", P), ("ema", P), ("n", i64), ("lr", f), ("beta1", d), ("beta2", d),
                                  ("eps", f), ("weight_decay", f), ("bc1", f), ("bc2", f), ("clip_coef", f), ("clip_coef_dev", P),
                                  ("ema_one_minus_decay", f), ("stream", P)]),
        "dst_dropout": ("int", [("x", P), ("y", P), ("n", i64), ("p", f), ("seed", u64), ("stream_id", u32), ("stream", P)]),
    }
    for name, (ret, params) in want.items():
        proto = (trn if name.startswith("dst_") else smp).prototypes[name]
        assert (proto.name, proto.ret, proto.params) == (name, ret, params), name
    table = {P: ctypes.c_void_p, "int": ctypes.c_int, i32: ctypes.c_int32, i64: ctypes.c_int64, u32: ctypes.c_uint32, u64: ctypes.c_uint64,
             f: ctypes.c_float, d: ctypes.c_double}
    assert trn.prototypes["dst_dropout"].argtypes == [table[t] for _, t in want["dst_dropout"][1]]
    assert trn.prototypes["dst_adamw_ema"].argtypes[7:10] == [ctypes.c_float, ctypes.c_double, ctypes.c_double]


def test_every_export_is_bound_with_its_signature():
    """Over both whole headers: the exports ARE the parsed prototypes, the totals are those of the headers, and every function of the loaded
    library carries the parsed ``restype`` and ``argtypes``.  The headers hold 81 prototypes with 682 parameters - counted independently of the
    parser below, as commas + 1 - of which 480 are pointers (481 stars: ``const float* const* ptrs`` has two)."""
    import __graft_entry__ as g
    from collections import Counter
    g.build()
    lib = E.load_library()
    abi, headers = _headers()
    kinds, n_params, n_by_commas = Counter(), 0, 0
    for hdr, prefix, n_fn in zip(headers, ("ds_", "dst_"), (31, 50)):
        assert hdr.exports(prefix) == list(hdr.prototypes) and len(hdr.prototypes) == n_fn
        n_by_commas += sum(text.count(",") + 1 for text in re.findall(r"\b(?:int|void)\s+%s\w+\s*\(([^()]*)\)\s*;" % prefix, hdr.text))
        for name, proto in hdr.prototypes.items():
            assert proto.params and all(t in abi._ARG_CTYPES for _, t in proto.params), name
            kinds.update(t for _, t in proto.params)
            n_params += len(proto.params)
            fn = getattr(lib, name)
            assert fn.restype is (None if proto.ret == "void" else ctypes.c_int), name
            assert len(fn.argtypes) == len(proto.params) and list(fn.argtypes) == proto.argtypes, name
    assert E.EXPORTS == headers[0].exports("ds_")
    assert n_params == n_by_commas == 682
    assert dict(kinds) == {"*": 480, "int32_t": 91, "int64_t": 48, "float": 39, "int": 13, "uint64_t": 5, "double": 4, "uint32_t": 2}
    assert [n for h in headers for n, p in h.prototypes.items() if p.ret == "void"] == ["ds_struct_sizes"]


@pytest.mark.parametrize("decl, param", [
    ("int ds_x(const float* a, size_t n, void* stream);", "size_t n"),               # a scalar type outside the table
    ("int ds_x(const float* a,\n         ds_layout L, void* stream);", "ds_layout L"),   # a struct by value
    ("int ds_x(int32_t n[4]);", "int32_t n[4]"),                                      # an array declarator
    ("int ds_x(unsigned int n);", "unsigned int n"),
])
def test_prototype_parser_refuses_what_it_does_not_know(decl, param):
    """A parameter that is neither a pointer nor a scalar of the table raises when the header is parsed, naming function and parameter:
    there is no default type."""
    abi, _ = _headers()
    ok = abi.Header("synthetic.h", "/* c */ int ds_y(const float* const* p, const int64_t n, double\n s); // c\nvoid ds_z(void);\n")
    assert ok.prototypes["ds_y"].params == [("p", "*"), ("n", "int64_t"), ("s", "double")] and ok.prototypes["ds_z"] == ("ds_z", "void", [])
    with pytest.raises(ValueError) as err:
        abi.Header("synthetic.h", "typedef struct ds_layout { int32_t B; } ds_layout;\n" + decl)
    assert "ds_x" in str(err.value) and param in str(err.value)


def test_ctypes_refuses_calls_that_disagree_with_the_header():
    """With ``argtypes`` set a wrong call never enters the library (every pointer here is NULL and P = 0: a call that did get through would
    return a status instead of raising).  A mistyped argument is ``ctypes.ArgumentError``; too few arguments are ctypes' plain ``TypeError``."""
    import __graft_entry__ as g
    g.build()
    lib = E.load_library()
    assert lib.ds_graph_hash_records(None, None, 0, None, None) == 0
    with pytest.raises(TypeError, match="at least 5 arguments"):                      # a missing argument
        lib.ds_graph_hash_records(None, None, 0, None)
    with pytest.raises(ctypes.ArgumentError, match="argument 3"):                     # a Python float where int64_t P is declared
        lib.ds_graph_hash_records(None, None, 0.0, None, None)
    with pytest.raises(ctypes.ArgumentError, match="argument 8"):                     # a c_int64 where int32_t max_nodes is declared
        lib.ds_graph_identity_records(None, None, 0, None, None, 0, None, ctypes.c_int64(0), None, None, None, None)
    with pytest.raises(ctypes.ArgumentError, match="argument 3"):                     # and a c_int32 where int64_t P is declared
        lib.ds_graph_hash_records(None, None, ctypes.c_int32(0), None, None)
    # what call sites do pass: ints, None, byref, ctypes arrays, the bytes of a packed struct - c_void_p takes them all
    size = ctypes.c_int64(-1)
    assert lib.ds_mmd_1d_workspace_bytes(3, ctypes.byref(size)) == 0 and size.value > 0
    assert ctypes.c_void_p.from_param(b"\0" * 8) is not None and ctypes.c_void_p.from_param((ctypes.c_int64 * 2)()) is not None


def test_call_sites_leave_the_argument_types_to_the_binder():
    """In the package, outside ``abi.py``: no scalar or pointer cast as a call argument (a by-reference out-parameter is the exception), and
    neither ``restype`` nor ``argtypes`` is set anywhere but in ``abi.Header.bind``."""
    root = os.path.dirname(os.path.abspath(E.__file__))
    cast = re.compile(r"\bC\.c_(?:int|int32|int64|uint32|uint64|float|double|void_p)\(")
    for name in sorted(os.listdir(root)):
        if not name.endswith(".py") or name == "abi.py":
            continue
        for no, line in enumerate(open(os.path.join(root, name)), 1):
            assert ".restype" not in line and ".argtypes" not in line, (name, no)
            if cast.search(line):
                assert re.match(r"\s*\w+ = C\.c_int64\(0\)$", line.rstrip()), (name, no, line)      # `size`, passed with byref
    src = open(os.path.join(root, "abi.py")).read()
    assert src.count(".restype =") == src.count(".argtypes =") == 1


def test_training_structs_parsed_from_the_header():
    """The binding packs the training C-ABI's argument structs in the layouts parsed from include/diffspectra_train.h: pinned to the
    layouts the kernels were validated with (the library checks the sizes at load time)."""
    from diffspectra_amd import train_engine as T
    expected = {
        "dst_gemm_args": "@PqqPqqPqPiiiiPqiiPiiPqPqfIQq",
        "dst_layout": "@iiiiPP",
        "dst_piece": "@PPiiqq",
        "dst_pair_chain_args": "@PPP PPPPq Pq iiii PPPPP q PPP f III Q PPPPPPPPPPP",
        "dst_pair_front_args": "@PPP PPq iiii PPPPPP PPPPPPP",
        "dst_dir_chain_args": "@PPP PPPq ii PPP PPPPPP",
        "dst_node_chain_args": "@PPP Pq iiii PPPPPPP f III Q PPPPPPPPP",
        "dst_dir_bwd_args": "@PPPPq PPPP PPq ii PP PPP",
        "dst_pair_bwd_args": "@PPPPq PPqP PPPPP PPq iiii PPPP f III Q PPPPPP",
        "dst_node_bwd_args": "@PPPPq PPqP PPPPP PPq iiii PPPP f III Q PPPPP",
    }
    assert {n: s.format for n, s in T.STRUCTS.items()} == {n: f.replace(" ", "") for n, f in expected.items()}
    assert sorted(T.STRUCT_NAMES) == sorted(expected)
    assert [f for f, _ in T.header_structs()["dst_pair_chain_args"]][-11:] == ["he", "xe1", "st", "ye1", "f3", "s3", "f4", "e_out", "X2", "ed", "ro"]
    assert ctypes.sizeof(T.DstLayout) == T.STRUCTS["dst_layout"].size and ctypes.sizeof(T.DstPiece) == T.STRUCTS["dst_piece"].size


def test_sampling_structs_parsed_from_the_header():
    """The sampling C-ABI's four argument structs are built from include/diffspectra_hip.h: pinned, field by field, to the layouts the
    kernels were validated with - a reordered header keeps every sizeof and would swap buffers silently."""
    from diffspectra_amd import abi
    assert (E.W_BLOCK_SLOTS, E.W_GLOBAL_SLOTS, E.W_NUM_SLOTS, E.NB) == (43, 38, 382, 8)
    assert len(E.BLOCK_SLOTS) == 44 and E.BLOCK_SLOTS[0] == "DS_BW_EDGE_EMB_W" and E.BLOCK_SLOTS[-2:] == ["DS_BW_EDGE_EMB_H", "DS_W_BLOCK_SLOTS"]
    assert len(E.GLOBAL_SLOTS) == 39 and E.GLOBAL_SLOTS[0] == "DS_GW_SIN_W" and E.GLOBAL_SLOTS[-2:] == ["DS_GW_ET2_C", "DS_W_GLOBAL_SLOTS"]
    expected = {
        "ds_weights": "@PP 382q ff",
        "ds_layout": "@iiiiii PPPPPPPP",
        "ds_workspace": "@" + 20 * "P",
        "ds_gemm_args": "@Pqiiq PP Pqiiq iiii Pqii PP",
    }
    assert {n: abi.SAMPLING.packer(n).format for n in abi.SAMPLING.structs} == {n: f.replace(" ", "") for n, f in expected.items()}
    names = lambda t: [f[0] for f in t._fields_]
    assert names(E.DsWeights) == ["base", "off_dev", "off", "edge_th", "spatial_cut_off"]
    assert names(E.DsLayout) == ["B", "N", "Nn", "Pp", "max_n", "_pad", "node_off", "pair_off", "node_dense", "node_mol", "pair_a", "pair_b",
                                 "pair_mol", "mol_by_size"]
    assert names(E.DsWorkspace) == E._WS_FIELDS == ["pos", "h", "e", "atom_hids", "edge_hids", "tfeat", "tmid", "temb_silu", "ada", "qkv", "ye",
                                                    "dist", "attn", "u", "ac", "ed", "lg", "tr", "adj", "flags"]
    assert names(E.DsGemmArgs) == ["A", "lda", "a_grp_rows", "_p0", "a_grp_stride", "Wp", "bias", "C", "ldc", "c_grp_rows", "_p1", "c_grp_stride",
                                   "M", "K", "N", "act", "R", "ldr", "r_grp_rows", "a_silu", "col_scale", "col_shift"]
    for t, n in ((E.DsWeights, "ds_weights"), (E.DsLayout, "ds_layout"), (E.DsWorkspace, "ds_workspace"), (E.DsGemmArgs, "ds_gemm_args")):
        assert ctypes.sizeof(t) == abi.SAMPLING.packer(n).size
    assert E.DsWeights.off.size == 382 * 8 and E.DsLayout.node_off.offset == 24


def test_training_surface_refuses_cpu():
    """Row N1 has no CPU path either: optimizer, loss function and graphs raise off the GPU."""
    from diffspectra_amd import losses as Lh, train_engine as T
    from diffspectra_amd.registry import create_model
    import diffspectra_amd.dmt  # noqa: F401
    cfg = qm9s_config("ir")
    model = create_model(cfg)
    with pytest.raises(RuntimeError):
        Lh.get_optimizer(cfg, model.parameters())
    with pytest.raises(RuntimeError):
        T.DmtTrainGraph({}, cfg, "cpu")
    cfg.model.dropout = 0.0
    from diffspectra_amd.noise_schedule import NoiseScheduleVP
    loss_fn = Lh.get_sde_graph_loss_fn(NoiseScheduleVP("cosine"), True, None, cfg)
    with pytest.raises(RuntimeError):
        loss_fn(model, {})
    q = Lh.Queue()
    q.add(3000)
    coef, allowed = Lh.clip_coefficient(18.0, q, 10.0)              # losses.py:33-44: allowed = min(1.5 mean + 2 std, max_grad)
    assert allowed == 10.0 and abs(coef - 10.0 / (18.0 + 1e-6)) < 1e-12 and q.items[0] == 10.0


def test_missing_library_fails_loudly(monkeypatch):
    monkeypatch.setattr(E, "_lib", None)
    monkeypatch.setattr(E, "LIB_PATH", "/nonexistent/libdiffspectra_hip.so")
    with pytest.raises(RuntimeError, match="no CPU/PyTorch fallback"):
        E.load_library()


def test_model_refuses_cpu():
    import diffspectra_amd.dmt  # noqa: F401
    from diffspectra_amd.registry import create_model
    cfg = qm9s_config("ir", device="cpu")
    model = create_model(cfg)
    a = filler.synthetic_state([3, 4], "cpu.x")
    with pytest.raises(RuntimeError, match="no CPU path"):
        model(torch.zeros(2), a[0], a[2], a[3], context=torch.zeros(2, 1, 3501), edge_x=a[1], noise_level=torch.zeros(2),
              cond_x=None, cond_edge_x=None)


def test_pack_linear_matches_kernel_indexing():
    """pack_linear vs the index formula the kernels use (wave_mma float4 fetch / wp_at)."""
    g = torch.Generator().manual_seed(0)
    for N, K in ((6, 128), (252, 64), (64, 68), (1024, 17)):
        W = torch.randn(N, K, generator=g)
        p = E.pack_linear(W)
        Kp, Np = (K + 7) // 8 * 8, (N + 31) // 32 * 32
        assert p.numel() == Kp * Np
        k = torch.arange(Kp).view(-1, 1)
        n = torch.arange(Np).view(1, -1)
        idx = (((k >> 3) * 2 + ((k >> 2) & 1)) * Np + n) * 4 + (k & 3)
        B = p[idx]
        want = torch.zeros(Kp, Np)
        want[:K, :N] = W.t()
        assert torch.equal(B, want)


def test_packed_weights_cover_every_parameter():
    cfg, sd = procedural_state_dict("ir")
    flat, off = E.pack_dmt_weights(sd)
    assert len(off) == E.W_NUM_SLOTS and len(set(off)) == len(off)
    assert all(o % 64 == 0 for o in off)
    assert torch.isfinite(flat).all()
    # every DMT (non-SpecFormer) parameter value must be recoverable from the packed buffer: check the totals
    n_dmt = sum(v.numel() for k, v in sd.items() if not k.startswith("cond_encoder.") and k != "cond_lin.weight" and k != "cond_lin.bias")
    assert int((flat != 0).sum()) >= int(0.999 * n_dmt)


def test_layout_tables():
    node_mask, edge_mask = filler.masks_from_n_atoms([3, 1, 5, 2])
    L = E.Layout(node_mask, "cpu")
    assert (L.B, L.N, L.Nn, L.Pp, L.max_n) == (4, 5, 11, 3 + 0 + 10 + 1, 5)
    t = {k: v.numpy() for k, v in L.t.items()}
    assert t["node_off"].tolist() == [0, 3, 4, 9, 11] and t["pair_off"].tolist() == [0, 3, 3, 13, 14]
    for m in range(4):
        n = t["node_off"][m + 1] - t["node_off"][m]
        for p in range(t["pair_off"][m], t["pair_off"][m + 1]):
            a, b = t["pair_a"][p] - t["node_off"][m], t["pair_b"][p] - t["node_off"][m]
            assert 0 <= a < b < n and t["pair_mol"][p] == m
            assert p - t["pair_off"][m] == a * (2 * n - a - 1) // 2 + (b - a - 1)   # the formula the kernels use
    L.check_edge_mask(edge_mask)
    bad = edge_mask.clone(); bad[0] = 1   # a diagonal entry
    with pytest.raises(ValueError):
        L.check_edge_mask(bad)


def test_factory_and_checkpoint_contract():
    """module.-prefixed state dict, strict load, EMA-style copy into parameters() order."""
    import diffspectra_amd.dmt  # noqa: F401
    from diffspectra_amd.registry import create_model, register_model
    cfg = qm9s_config("allspectra", device="cpu")
    model = create_model(cfg)
    sd = model.state_dict()
    assert len(sd) == 435 and all(k.startswith("module.") for k in sd)
    trainable = [p for p in model.parameters() if p.requires_grad]
    assert len(trainable) == 414 and sum(p.numel() for p in model.parameters()) == 39630619
    model.load_state_dict(filler.fill_state_dict(sd), strict=True)
    with pytest.raises(ValueError):
        register_model(name="DMT")(type("X", (), {}))


def test_pretrained_specformer_key_mapping():
    """dmt.py:268-303: Lightning-style keys → cond_encoder.*"""
    import diffspectra_amd.dmt as D
    cfg = qm9s_config("ir", device="cpu")
    m = D.DMT(cfg)
    src = {}
    for k, v in m.cond_encoder.state_dict().items():
        key = f"model.representation_model.{k}"
        src[key] = torch.full_like(v, 0.25) if v.dtype.is_floating_point else v
    n = m.load_pretrained_specformer_state(src)
    assert n == len(m.cond_encoder.state_dict())
    assert float(m.cond_encoder.head.linear.weight[0, 0]) == 0.25


def test_sampler_surface():
    from diffspectra_amd import sampling as S
    from diffspectra_amd.noise_schedule import NoiseScheduleVP
    cfg = qm9s_config("ir", steps=7)
    ns = NoiseScheduleVP("cosine", continuous_beta_0=0.1, continuous_beta_1=20.0)
    assert ns.T == 0.9946
    smp = S._make_sampler(cfg, ns, 1e-3, 1.0)
    assert smp.coefficient_table().shape == (7, 4)
    with pytest.raises(TypeError):
        smp.sampling(lambda *a, **k: None, torch.zeros(1, 2, 9), torch.ones(1, 2, 1), torch.ones(4, 1), torch.zeros(1, 2, 2, 2), None)
    bad = cfg.clone(); bad.sampling.method = "ode"
    with pytest.raises(ValueError, match="Invalid sampling method"):
        S.get_cond_sampling_eval_fn(bad, ns, 4, 4, None, [])
    nm, em = S.build_masks([2, 3], 2, "cpu")
    want_nm, want_em = filler.masks_from_n_atoms([2, 3])
    assert torch.equal(nm, want_nm) and torch.equal(em, want_em)


def test_packed_spectra_table():
    """N3 (conditioning side): the HBM-resident table hands a round exactly what per-item assembly would."""
    from types import SimpleNamespace
    from diffspectra_amd.dataset_pack import PackedSpectraTable
    M = 9
    raw = [filler.uniform(f"pack.{n}", (M, 1, L)) * 50.0 for n, L in zip(("uv", "ir", "raman"), (701, 3501, 3501))]
    n_atoms = filler.sample_n_atoms(M, seed=4).tolist()
    ds = [SimpleNamespace(uv=raw[0][i], ir=raw[1][i], raman=raw[2][i], num_atom=torch.tensor(n_atoms[i]),
                          pos=torch.full((n_atoms[i], 3), float(i)), rdmol=f"m{i}") for i in range(M)]
    tab = PackedSpectraTable.from_dataset(ds, "allspectra", normalize=True)
    assert len(tab) == M
    ids = torch.tensor([7, 2, 2, 5])
    ctx, n_nodes, pos, mols = tab.batch(ids, "allspectra")
    assert n_nodes == [n_atoms[i] for i in ids.tolist()] and mols == ["m7", "m2", "m2", "m5"]
    assert all(torch.equal(p, ds[i].pos) for p, i in zip(pos, ids.tolist()))
    for k in range(3):      # log10(x + 1) of the reference transform (build_dataset.py:141-148), stacked like sampling.py:404-420
        want = torch.stack([torch.log10(raw[k][i] + 1) for i in ids.tolist()])
        assert ctx[k].shape == want.shape and torch.equal(ctx[k], want)
    it = tab[5]             # dataset surface kept for code written against the reference's ds[i]
    assert int(it.num_atom) == n_atoms[5] and it.rdmol == "m5" and torch.equal(it.ir, torch.log10(raw[1][5] + 1))
    ir_only = PackedSpectraTable.from_dataset(ds, "ir")
    c1, n1, _, _ = ir_only.batch([0, 8], "ir")
    assert torch.equal(c1, torch.stack([raw[1][0], raw[1][8]])) and n1 == [n_atoms[0], n_atoms[8]]
    with pytest.raises(ValueError):
        ir_only.batch([0], "allspectra")
    with pytest.raises(ValueError):
        PackedSpectraTable([raw[0][:, :, :10], None, None], torch.tensor(n_atoms))


def _write_processed_qm9s(proc_dir, mols, layout):
    """Write data_qm9_allspectra.pt + split file the way InMemoryDataset.collate + torch.save do, WITHOUT PyG / RDKit: classes
    named like theirs live in throw-away modules while pickling (PyG 2.4.0: Data.__dict__ = {_edge_attr_cls, _tensor_attr_cls,
    _store}, GlobalStorage.__getstate__ = its __dict__ with _parent resolved; PyG 1.x: the tensors directly in Data.__dict__)."""
    import sys
    import types
    names = ["torch_geometric", "torch_geometric.data", "torch_geometric.data.data", "torch_geometric.data.storage",
             "rdkit", "rdkit.Chem", "rdkit.Chem.rdchem"]
    mods = {n: types.ModuleType(n) for n in names}

    def cls(module, name):
        c = type(name, (), {"__module__": module})
        setattr(mods[module], name, c)
        return c
    Data, Storage, Mol = cls("torch_geometric.data.data", "Data"), cls("torch_geometric.data.storage", "GlobalStorage"), cls("rdkit.Chem.rdchem", "Mol")
    EdgeAttr, TensorAttr = cls("torch_geometric.data.data", "DataEdgeAttr"), cls("torch_geometric.data.data", "DataTensorAttr")
    cat = lambda k, dim=0: torch.cat([m[k] for m in mols], dim)
    cum = lambda sizes: torch.tensor([0] + list(np.cumsum(sizes)), dtype=torch.int64)
    M = len(mols)
    rdmols = []
    for i in range(M):
        r = Mol()
        r.tag = f"mol{i}"
        rdmols.append(r)
    mapping = {"atom_type": cat("atom_type"), "pos": cat("pos"), "edge_index": cat("edge_index", 1), "edge_type": cat("edge_type"),
               "uv": cat("uv"), "ir": cat("ir"), "raman": cat("raman"),
               "num_atom": torch.tensor([m["pos"].shape[0] for m in mols]), "idx": torch.arange(M), "rdmol": rdmols}
    n = [m["pos"].shape[0] for m in mols]
    ne = [m["edge_type"].shape[0] for m in mols]
    one = torch.arange(M + 1)
    slices = {"atom_type": cum(n), "pos": cum(n), "edge_index": cum(ne), "edge_type": cum(ne), "uv": one, "ir": one, "raman": one,
              "num_atom": one, "idx": one, "rdmol": one}
    if "fc" in mols[0]:                               # per-atom formal charges (qm9s_dataset.py:267)
        mapping["fc"], slices["fc"] = cat("fc"), cum(n)
    data = Data()
    if layout == "pyg2":
        st = Storage()
        st.__dict__.update({"_key": None, "_mapping": mapping, "_parent": data})
        data.__dict__.update({"_edge_attr_cls": EdgeAttr, "_tensor_attr_cls": TensorAttr, "_store": st})
    else:
        data.__dict__.update(mapping)
    os.makedirs(proc_dir, exist_ok=True)
    saved = {k: sys.modules.get(k) for k in names}
    sys.modules.update(mods)
    try:
        torch.save((data, slices), os.path.join(proc_dir, "data_qm9_allspectra.pt"))
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    perm = np.random.RandomState(0).permutation(M)
    torch.save({"first_train": perm[:2], "second_train": perm[2:4], "valid": perm[4:6], "test": perm[6:]},
               os.path.join(proc_dir, "split_dict_diffspectra_qm9.pt"))
    return perm


@pytest.mark.parametrize("layout", ["pyg2", "pyg1"])
def test_processed_qm9s_reader(tmp_path, layout):
    """N3 (on-disk side): data_qm9_allspectra.pt + split_dict_diffspectra_qm9.pt -> the sampler's table, item for item what
    ``dataset.index_select(split['test'])[i]`` + EdgeComSpectraTransform give (qm9s_dataset.py:153,306-312,357-361;
    build_dataset.py:36-42,141-148), read without PyG or RDKit."""
    from diffspectra_amd.qm9s_reader import ProcessedQM9S
    M = 11
    n_atoms = filler.sample_n_atoms(M, seed=9).tolist()
    mols = []
    for i, n in enumerate(n_atoms):
        ne = 2 * max(n - 1, 0)
        mols.append({"atom_type": torch.randint(0, 5, (n,)), "pos": filler.uniform(f"rd.pos{i}", (n, 3)),
                     "edge_index": torch.randint(0, max(n, 1), (2, ne)), "edge_type": torch.randint(1, 4, (ne,)),
                     "uv": filler.uniform(f"rd.uv{i}", (1, 701)).abs() * 30, "ir": filler.uniform(f"rd.ir{i}", (1, 3501)).abs() * 30,
                     "raman": filler.uniform(f"rd.ra{i}", (1, 3501)).abs() * 30})
    perm = _write_processed_qm9s(str(tmp_path / "processed"), mols, layout)
    ds = ProcessedQM9S(str(tmp_path))                       # the dataset root, as config.data.root
    assert len(ds) == M and sorted(ds.splits) == ["first_train", "second_train", "test", "valid"]
    test_ids = perm[6:].tolist()
    tab = ds.packed_table("allspectra", split="test")
    assert len(tab) == len(test_ids)
    for i, j in enumerate(test_ids):
        it = tab[i]
        assert int(it.num_atom) == n_atoms[j] and torch.equal(it.pos, mols[j]["pos"])
        for name in ("uv", "ir", "raman"):
            assert torch.equal(getattr(it, name), torch.log10(mols[j][name] + 1))
        assert type(it.rdmol).__name__ == "Mol" and it.rdmol._state["tag"] == f"mol{j}"      # opaque, but the right molecule
        assert torch.equal(ds.item_field("edge_index", j), mols[j]["edge_index"])           # concatenated along dim 1
        assert torch.equal(ds.item_field("atom_type", j), mols[j]["atom_type"])
    ctx, n_nodes, pos, _ = tab.batch([2, 0], "allspectra")
    assert n_nodes == [n_atoms[test_ids[2]], n_atoms[test_ids[0]]] and ctx[1].shape == (2, 1, 3501)
    assert torch.equal(ctx[0][1, 0], torch.log10(mols[test_ids[0]]["uv"][0] + 1))
    raw = ds.packed_table("ir", split="valid", normalize=False)
    assert torch.equal(raw[1].ir, mols[perm[5]]["ir"]) and raw.spectra[0] is None
    assert len(ds.packed_table("ir", split=None)) == M
    with pytest.raises(KeyError):
        ds.split("train")
    with pytest.raises(FileNotFoundError):
        ProcessedQM9S(str(tmp_path / "nowhere"))


def test_batched_stability_needs_the_hip_engine():
    """N4 has no PyTorch implementation: without an engine the batched stability check refuses."""
    from diffspectra_amd.stability import check_stability_batch
    with pytest.raises(RuntimeError):
        check_stability_batch(torch.zeros(1, 2, 3), torch.zeros(1, 2, dtype=torch.long), torch.ones(1, 2))


def test_build_reports_on_stderr_only(tmp_path, capsys):
    """bench.py calls build() and its stdout must stay ONE JSON line: a rebuild on the benchmark box (sources newer than the
    library) may only talk on stderr."""
    import __graft_entry__ as g
    obj = str(tmp_path / "x.o")
    src = str(tmp_path / "x.hip")
    open(src, "w").write("// empty\n")
    g._compile("/bin/true", src, obj, ["-O3"])
    cap = capsys.readouterr()
    assert cap.out == "" and "[build]" in cap.err
    assert open(obj + ".flags").read() == "-O3"
    with pytest.raises(FileNotFoundError):                   # a dependency that does not exist is an error, not an empty digest
        g._digest([str(tmp_path / "missing.h")])


def test_bf16_weight_table_and_concatenated_weight_plan():
    """The one table of the fused chains' bf16 weight copies (name, shape, source, transposed) and the plan of the concatenated buffers:
    pinned to what the kernels were validated with - per block the twelve straight copies, then the nine transposed ones, in this order
    (it is the order of the device table of ``dst_pack_bf16_pieces``)."""
    from diffspectra_amd import train_engine as T
    expected = [("W3", (128, 64), False), ("W4", (64, 128), False), ("Wed", (256, 128), False), ("Wro", (16, 64), False), ("Wee", (64, 128), False),
                ("Wte", (512, 64), False), ("W0", (256, 256), False), ("W2", (3, 256), False), ("F1", (512, 256), False), ("F2", (256, 512), False),
                ("Wac", (512, 256), False), ("Wn", (64, 256), False), ("W0T", (256, 256), True), ("WedT", (128, 256), True), ("WroT", (64, 16), True),
                ("W4T", (128, 64), True), ("W3T", (64, 128), True), ("WacT", (256, 512), True), ("WnT", (256, 64), True), ("F2T", (512, 256), True),
                ("F1T", (256, 512), True)]
    assert [(n, sh, tr) for n, sh, _, tr in T.BF16_WEIGHTS] == expected
    # a transposed copy has the source of the straight one and its shape reversed
    by_name = {n: (sh, src) for n, sh, src, _ in T.BF16_WEIGHTS}
    for n, sh, src, tr in T.BF16_WEIGHTS:
        if tr:
            straight = {"F1T": "F1", "F2T": "F2"}.get(n, n[:-1])
            assert by_name[straight] == (sh[::-1], src), n
    p = {f"e_block_3.{k}.weight": k for k in ("ff_linear3", "equi_update.coord_mlp.0")}
    p.update({"edge_3.weight": "edge", "node_3.weight": "node"})
    assert T._bf16_source(by_name["W3"][1], 3, p, {}) == "ff_linear3" and T._bf16_source(by_name["Wro"][1], 3, p, {}) == "edge"
    assert T._bf16_source(by_name["Wac"][1], 3, p, {"Wac": list("abcdefgh")}) == "d"
    w = torch.arange(256 * 640.0).reshape(256, 640)
    assert torch.equal(T._bf16_source(by_name["WedT"][1], 3, {"e_block_3.equi_update.input_lin.weight": w}, {}), w[:, 512:640])
    bufs, pieces = T.DmtTrainGraph.cat_plan()
    assert bufs == [("Wada", (T.ADA, 1024)), ("bada", (T.ADA,)), ("Wqkv", (8, 768, 256)), ("bqkv", (8, 768)), ("Wte", (8, 512, 64)), ("Wac", (8, 512, 256))]
    assert len(pieces) == 8 * 18 + 2
    for i in range(8):
        blk = pieces[18 * i:18 * (i + 1)]
        o = i * T.ADA_STRIDE + T.NODE_OFF
        assert blk[0] == ("Wada", (slice(o, o + 1536),), f"e_block_{i}.node_time_mlp.1.weight")
        assert blk[8] == ("Wqkv", (i, slice(0, 252)), f"e_block_{i}.attn_mpnn.lin_query.weight")
        assert blk[13] == ("bqkv", (i, slice(512, 768)), f"e_block_{i}.attn_mpnn.lin_value.bias")
        assert blk[14:16] == [("Wte", (i, slice(0, 252)), f"e_block_{i}.attn_mpnn.lin_edge0.weight"),
                              ("Wte", (i, slice(256, 512)), f"e_block_{i}.attn_mpnn.lin_edge1.weight")]
        assert blk[-1] == ("Wac", (i, slice(256, 512)), (f"e_block_{i}.equi_update.input_lin.weight", slice(256, 512)))
        assert [b for b, _, _ in blk] == ["Wada", "bada"] * 4 + ["Wqkv", "bqkv"] * 3 + ["Wte", "Wte", "Wac", "Wac"]
    assert pieces[-2:] == [("Wada", (slice(T.ADA_TOP, T.ADA_TOP + 2),), "dist_layer.time_mlp.1.weight"),
                           ("bada", (slice(T.ADA_TOP, T.ADA_TOP + 2),), "dist_layer.time_mlp.1.bias")]


def test_block_slots_name_the_adaln_columns_and_dropout_streams():
    """``train_engine.BLOCKS[i]`` names the columns of the adaLN table and the Philox streams of block ``i`` once, for the forward and the
    backward in both forms: every slot equals the literal offset the call sites used to spell out."""
    from diffspectra_amd import train_engine as T
    assert len(T.BLOCKS) == T.NB == 8
    for i, k in enumerate(T.BLOCKS):
        a0 = i * T.ADA_STRIDE
        n, e, q = a0 + T.NODE_OFF, a0 + T.EDGE_OFF, a0 + T.EQUI_OFF
        assert (k.i, k.bp) == (i, f"e_block_{i}.")
        assert (*k.node.ln1, k.node.gate1, *k.node.ln2, k.node.gate2) == (n, n + 256, n + 512, n + 768, n + 1024, n + 1280)
        assert (*k.edge.ln1, k.edge.gate1, *k.edge.ln2, k.edge.gate2) == (e, e + 64, e + 128, e + 192, e + 256, e + 320)
        assert k.equi_ln == (q, q + 256) and k.dist == a0 + T.DIST_OFF
        assert [k.drop(j) for j in range(4)] == [(4 * i, 512), (4 * i + 1, 256), (4 * i + 2, 128), (4 * i + 3, 64)]
    # the slots of a block lie inside its stride of the table, the last block's below the top-level distance slot
    assert T.BLOCKS[-1].node.gate2 + 256 <= T.ADA_TOP and T.BLOCKS[-1].edge.gate2 + 64 <= T.ADA_TOP and T.ADA_TOP + 2 <= T.ADA
