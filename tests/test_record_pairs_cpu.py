"""No GPU: the "record pairs" contract of include/diffspectra_hip.h that ``ds_match_records``, ``ds_graph_identity_records`` and
``ds_mces_records`` share (``ds_graph_hash_records`` where a rule applies) - the argument check of the C entry points, called through ctypes,
and the record layout, stated once in the header and compared here with the mirror's own numbers and with what the packer writes.

Every call below must be refused or launch nothing: the refusals return before the device is touched, so the pointers are small fake
addresses that are never dereferenced.  No combination that would pass every check is ever passed."""
import ctypes as C

import numpy as np
import pytest
import torch

from diffspectra_amd import engine as E, shard
from tests import structure_mirror as SM

OK, ERR_ARG = 0, -1
FAKE = 0x1000                        # a 4-byte aligned address that is nobody's memory
# entry point -> (scalars that pass the entry point's own checks, number of output pointers)
PAIR_ENTRIES = {
    "ds_match_records": ((C.c_float(5.0), C.c_int32(3)), 6),
    "ds_graph_identity_records": ((C.c_int32(16),), 3),
    "ds_mces_records": ((C.c_int32(1), C.c_int32(16)), 5),
}
ALL_ENTRIES = list(PAIR_ENTRIES) + ["ds_graph_hash_records"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return E.load_library()


def _call(lib, name, P, M=1, outputs=None, **pointers):
    """The entry point with fake pointers everywhere except where ``pointers`` (``prb_rec``, ``prb_n``, ``ref_rec``, ``ref_n``, ``ref_index``;
    ``rec`` and ``n`` of the hash) or ``outputs`` (a list of addresses) say otherwise; ``None`` is NULL."""
    ptr = lambda key: C.c_void_p(pointers.get(key, FAKE))
    if name == "ds_graph_hash_records":
        out = [FAKE] if outputs is None else outputs
        return lib.ds_graph_hash_records(ptr("rec"), ptr("n"), C.c_int64(P), C.c_void_p(out[0]), C.c_void_p(None))
    scalars, n_out = PAIR_ENTRIES[name]
    out = [FAKE] * n_out if outputs is None else outputs
    return getattr(lib, name)(ptr("prb_rec"), ptr("prb_n"), C.c_int64(P), ptr("ref_rec"), ptr("ref_n"), C.c_int64(M), ptr("ref_index"), *scalars,
                              *(C.c_void_p(o) for o in out), C.c_void_p(None))


def _tables(name):
    return ("rec", "n") if name == "ds_graph_hash_records" else ("prb_rec", "prb_n", "ref_rec", "ref_n")


def _n_outputs(name):
    return 1 if name == "ds_graph_hash_records" else PAIR_ENTRIES[name][1]


@pytest.mark.parametrize("name", ALL_ENTRIES)
def test_no_pairs_launch_nothing(lib, name):
    nulls = {key: None for key in _tables(name) + ("ref_index",)}
    assert _call(lib, name, 0, M=0, outputs=[None] * _n_outputs(name), **nulls) == OK


@pytest.mark.parametrize("name", ALL_ENTRIES)
def test_sizes_out_of_range_are_refused(lib, name):
    assert _call(lib, name, -1) == ERR_ARG
    assert _call(lib, name, 2 ** 31, M=2 ** 31) == ERR_ARG
    if name in PAIR_ENTRIES:
        assert _call(lib, name, 1, M=-1) == ERR_ARG
        assert _call(lib, name, 0, M=-1) == ERR_ARG                     # the sizes are checked before "P = 0 launches nothing"


@pytest.mark.parametrize("name", ALL_ENTRIES)
def test_every_required_pointer_is_required(lib, name):
    for key in _tables(name):
        assert _call(lib, name, 1, **{key: None}) == ERR_ARG, key
    for k in range(_n_outputs(name)):
        out = [FAKE] * _n_outputs(name)
        out[k] = None
        assert _call(lib, name, 1, outputs=out) == ERR_ARG, f"output {k}"


@pytest.mark.parametrize("name", list(PAIR_ENTRIES))
def test_identity_pairing_needs_a_row_for_every_pair(lib, name):
    assert _call(lib, name, 2, M=1, ref_index=None) == ERR_ARG


@pytest.mark.parametrize("name", ALL_ENTRIES)
def test_misaligned_tables_are_refused(lib, name):
    for key in _tables(name)[::2]:                                      # the record tables: rec, or prb_rec and ref_rec
        assert _call(lib, name, 1, **{key: FAKE + 1}) == ERR_ARG, key


def test_layout_of_header_mirror_and_packer():
    """The header's offsets = the mirror's plain numbers = where ``shard.pack_records_u8`` puts each field; unpack inverts pack."""
    K = E.CONSTS
    assert (K["DS_MAX_ATOMS"], K["DS_RECORD_BYTES"]) == (SM.W, SM.RECORD_BYTES) == (shard.RECORD_ATOMS, shard.RECORD_BYTES) == (29, 1248)
    assert tuple(K["DS_REC_" + k] for k in ("POS", "TYPE", "FC", "BOND", "BOND_END")) == (SM.POS, SM.TYPE, SM.FC, SM.BOND, SM.BOND_END)
    assert SM.BOND_END <= SM.RECORD_BYTES and SM.RECORD_BYTES % 4 == 0
    W = SM.W
    pos = (np.arange(W * 3, dtype=np.float32) + 0.5).reshape(1, W, 3)                 # distinct values in every field
    types = (np.arange(W, dtype=np.int64) + 1).reshape(1, W)
    fc = -(np.arange(W, dtype=np.int64) + 1).reshape(1, W)
    bond = (np.arange(W * W, dtype=np.int64) % 251 + 1).reshape(1, W, W)
    rec_t = shard.pack_records_u8(*(torch.as_tensor(x) for x in (pos, types, fc, bond)))
    assert rec_t.shape == (1, SM.RECORD_BYTES) and rec_t.dtype == torch.uint8
    rec = rec_t[0].numpy()
    assert np.array_equal(rec[SM.POS:SM.TYPE].view(np.float32), pos.reshape(-1))
    assert np.array_equal(rec[SM.TYPE:SM.FC], types.reshape(-1).astype(np.uint8))
    assert np.array_equal(rec[SM.FC:SM.BOND].view(np.int8), fc.reshape(-1).astype(np.int8))
    assert np.array_equal(rec[SM.BOND:SM.BOND_END], bond.reshape(-1).astype(np.uint8))
    assert not rec[SM.BOND_END:].any()
    back = shard.unpack_records_u8(rec_t)
    for got, want in zip(back, (pos, types, fc, bond)):
        assert got.shape == want.shape and np.array_equal(got.numpy(), want)
    mol = SM.mol_from_record(rec, W)                                                  # and the mirror reads the same fields
    assert np.array_equal(mol["pos"], pos[0]) and np.array_equal(mol["type"], types[0]) and np.array_equal(mol["fc"], fc[0])
    assert np.array_equal(mol["bond"], bond[0])
