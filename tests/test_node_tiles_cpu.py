"""CPU: the C-ABI surface of the launch-form switches (include/diffspectra_tiles.h).  ``ds_set_node_tile`` only stores a process-global
choice, so its contract - previous value returned, anything but 32 / 64 means "choose by size" - is checked here without a GPU; what the
two forms compute is tests/test_node_tiles_gpu.py."""
import ctypes as C

import pytest

from diffspectra_amd import abi, engine as E


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return E.load_library()


def test_header_declares_and_library_exports_the_switch(lib):
    assert list(abi.TILES.prototypes) == abi.TILES.exports("ds_") == ["ds_set_node_tile"]
    proto = abi.TILES.prototypes["ds_set_node_tile"]
    assert (proto.ret, proto.params) == ("int", [("rows", "int")])
    assert not abi.TILES.structs and not abi.TILES.enums
    assert "ds_set_node_tile" not in abi.SAMPLING.prototypes          # declared once
    fn = lib.ds_set_node_tile
    assert fn.restype is C.c_int and list(fn.argtypes) == [C.c_int]   # bound from the header


def test_setter_returns_the_previous_value_and_normalises(lib):
    prev = lib.ds_set_node_tile(32)
    try:
        assert lib.ds_set_node_tile(64) == 32
        assert lib.ds_set_node_tile(-1) == 64
        assert lib.ds_set_node_tile(48) == -1          # neither form: choose by size
        assert lib.ds_set_node_tile(0) == -1
        assert lib.ds_set_node_tile(32) == -1
        with pytest.raises(C.ArgumentError):
            lib.ds_set_node_tile(64.0)
    finally:
        lib.ds_set_node_tile(prev)
