"""The one description of the C-ABI on the Python side: the headers (``include/diffspectra_hip.h`` for sampling, ``include/diffspectra_train.h``
for training, ``include/diffspectra_sets.h`` for the set-against-set analytics, ``include/diffspectra_valence.h`` for the valence analytics, ``include/diffspectra_groups.h`` for the functional groups, ``include/diffspectra_scaffold.h`` for the scaffolds, ``include/diffspectra_smiles.h`` for the SMILES strings, ``include/diffspectra_substructure.h`` for the substructure matcher, ``include/diffspectra_stereo.h`` for the stereo-aware identity, ``include/diffspectra_brics.h`` for the BRICS fragments, ``include/diffspectra_mobile.h`` for the mobile-hydrogen normal form, ``include/diffspectra_key.h`` for the key-level identity, ``include/diffspectra_fraggle.h`` for the Fraggle similarity, ``include/diffspectra_rmsd.h`` for the symmetry-corrected RMSD, ``include/diffspectra_reader.h`` for the SMILES reader, ``include/diffspectra_tiles.h`` for the launch-form switches, ``include/diffspectra_step.h`` for the uniform-step entry points, ``include/diffspectra_solver.h`` for the multistep solver update) are read here and nowhere else.  ``engine`` and ``train_engine`` build their ctypes types and ``struct`` packers from what this
module parsed, so a struct is described once, in its header; the library reports its ``sizeof``s and the loaders compare.  The function
prototypes are read too: ``Header.bind`` gives every export its ``argtypes``, so a call site passes plain Python numbers and data pointers and
ctypes refuses a call with too few arguments or with one of the wrong kind."""
from __future__ import annotations

import ctypes as C
import os
import re
import struct as _struct
from typing import Dict, List, NamedTuple, Tuple

_INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")

_FIELD_CODES = {"int64_t": "q", "int32_t": "i", "uint32_t": "I", "uint64_t": "Q", "float": "f"}
_CTYPES = {"P": C.c_void_p, "q": C.c_int64, "i": C.c_int32, "I": C.c_uint32, "Q": C.c_uint64, "f": C.c_float}
# by-value parameter types of the exported functions; "*" stands for every pointer, whatever it points to: call sites pass addresses as ints,
# None, byref(...), ctypes arrays and the bytes of a packed argument struct, and c_void_p takes all of them
_ARG_CTYPES = {"*": C.c_void_p, "int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
               "float": C.c_float, "double": C.c_double}


class Prototype(NamedTuple):
    """One exported function: ``ret`` is ``"int"`` or ``"void"``, ``params`` are ``(name, C type)`` with the type a key of ``_ARG_CTYPES``."""
    name: str
    ret: str
    params: List[Tuple[str, str]]

    @property
    def argtypes(self):
        return [_ARG_CTYPES[t] for _, t in self.params]


def ptr(t):
    """Data pointer of a tensor, 0 (NULL) for ``None``: an int both for a ``c_void_p`` parameter and for a ``P`` field of a ``struct`` packer,
    which refuses ``None``."""
    return 0 if t is None else t.data_ptr()


class Header:
    """One parsed header: ``enums`` {enum name: enumerator names in order}, ``consts`` {name: int} of the enumerators and of every ``#define``
    that evaluates to an integer, ``reals`` {name: float} of every ``#define`` of a decimal literal, ``structs`` {struct name: [(field, struct code)]} of every ``typedef struct``, ``prototypes`` {function
    name: Prototype} of every exported function."""

    def __init__(self, file_name: str, text: str = None):
        """``text``: parse this instead of the file's contents (the tests feed the parser malformed headers)."""
        self.path = os.path.join(_INCLUDE, file_name)
        if text is None:
            with open(self.path) as f:
                text = f.read()
        self.text = re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)      # without its comments
        self.enums: Dict[str, List[str]] = {}
        self.consts: Dict[str, int] = {}
        for name, body in re.findall(r"enum\s+(\w+)\s*\{(.*?)\}", self.text, flags=re.S):
            value = -1
            self.enums[name] = []
            for item in filter(None, (t.strip() for t in body.split(","))):
                ident, _, given = (p.strip() for p in item.partition("="))
                value = int(given, 0) if given else value + 1
                self.enums[name].append(ident)
                self.consts[ident] = value
        defs = dict(re.findall(r"#define\s+(\w+)\s+(\(?[-\w\s\*\+\(\)]+?\)?)\s*$", self.text, flags=re.M))
        for _ in range(4):  # resolve nested defines
            for k, v in defs.items():
                if k not in self.consts:
                    try:
                        self.consts[k] = int(eval(v, {"__builtins__": {}}, self.consts))
                    except Exception:
                        pass
        self.reals: Dict[str, float] = {k: float(v) for k, v in re.findall(r"#define\s+(\w+)\s+(\d+\.\d+(?:[eE][-+]?\d+)?)\s*$", self.text, flags=re.M)}
        self.structs = {name: self._fields(body) for name, body in re.findall(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}", self.text, flags=re.S)}
        self.prototypes = {name: Prototype(name, ret, self._params(name, params))
                           for ret, name, params in re.findall(r"^\s*(int|void)\s+(\w+)\s*\(([^()]*)\)\s*;", self.text, flags=re.M)}

    def _fields(self, body: str) -> List[Tuple[str, str]]:
        """Any pointer is ``P``, scalars map through ``_FIELD_CODES``, a fixed array ``t x[N]`` is ``N`` copies of its scalar (``"8q"``; N an
        integer or a parsed constant); a declaration may list several fields (``int32_t a, b;``, ``float *x, *y;``)."""
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            typ, rest = re.fullmatch(r"(?:const\s+)?(\w+)\s*(.*)", decl, flags=re.S).groups()
            for f_ in rest.split(","):
                name, length = re.fullmatch(r"([*\s]*\w+)\s*(?:\[\s*(\w+)\s*\])?", f_.strip()).groups()
                code = "P" if name.startswith("*") else _FIELD_CODES[typ]
                if length is not None:
                    code = f"{self.consts[length] if length in self.consts else int(length)}{code}"
                fields.append((name.lstrip("* "), code))
        return fields

    @staticmethod
    def _params(function: str, text: str) -> List[Tuple[str, str]]:
        """Anything with a ``*`` is a pointer; every other parameter is ``[const] <scalar of _ARG_CTYPES> <name>``.  Whatever else a header may
        come to declare (a struct by value, an array, an unknown type) raises here: there is no default type."""
        params = []
        if text.strip() == "void":
            return params
        for decl in (d.strip() for d in text.split(",")):
            if "*" in decl:
                typ, m = "*", re.fullmatch(r"[\w\s*]*?(\w+)", decl)
            else:
                m = re.fullmatch(r"(?:const\s+)?(\w+)\s+(\w+)", decl)
                typ, m = (m.group(1), m) if m else (None, None)
            if m is None or typ not in _ARG_CTYPES:
                raise ValueError(f"{function}: parameter '{decl}' is neither a pointer nor one of the scalar types {sorted(_ARG_CTYPES)[1:]}")
            params.append((m.group(m.lastindex), typ))
        return params

    def exports(self, prefix: str) -> List[str]:
        """The functions the header declares whose names start with ``prefix``."""
        return [name for name in self.prototypes if name.startswith(prefix)]

    def bind(self, lib: C.CDLL) -> None:
        """``restype`` and ``argtypes`` of every function of the header on ``lib`` (AttributeError if the library lacks one): from here on
        ctypes converts plain Python arguments as the header says and refuses a missing or a mistyped one before the library is entered (a
        surplus one it still lets through: these are cdecl functions)."""
        for p in self.prototypes.values():
            fn = getattr(lib, p.name)
            fn.restype = None if p.ret == "void" else C.c_int
            fn.argtypes = p.argtypes

    def packer(self, name: str) -> _struct.Struct:
        return _struct.Struct("@" + "".join(code for _, code in self.structs[name]))      # native alignment: the C compiler's layout

    def ctypes_struct(self, name: str):
        def ctype(code):
            return _CTYPES[code[-1]] * int(code[:-1]) if len(code) > 1 else _CTYPES[code]
        return type(name, (C.Structure,), {"_fields_": [(f_, ctype(code)) for f_, code in self.structs[name]]})


SAMPLING = Header("diffspectra_hip.h")
TRAINING = Header("diffspectra_train.h")
SETS = Header("diffspectra_sets.h")
VALENCE = Header("diffspectra_valence.h")
GROUPS = Header("diffspectra_groups.h")
SCAFFOLD = Header("diffspectra_scaffold.h")
SMILES = Header("diffspectra_smiles.h")
SUBSTRUCTURE = Header("diffspectra_substructure.h")
STEREO = Header("diffspectra_stereo.h")
BRICS = Header("diffspectra_brics.h")
MOBILE = Header("diffspectra_mobile.h")
KEY = Header("diffspectra_key.h")
FRAGGLE = Header("diffspectra_fraggle.h")
RMSD = Header("diffspectra_rmsd.h")
READER = Header("diffspectra_reader.h")
TILES = Header("diffspectra_tiles.h")
STEP = Header("diffspectra_step.h")
SOLVER = Header("diffspectra_solver.h")
