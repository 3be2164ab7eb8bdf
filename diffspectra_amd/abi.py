"""The one description of the C-ABI on the Python side: both headers (``include/diffspectra_hip.h`` for sampling, ``include/diffspectra_train.h``
for training) are read here and nowhere else.  ``engine`` and ``train_engine`` build their ctypes types and ``struct`` packers from what this
module parsed, so a struct is described once, in its header; the library reports its ``sizeof``s and the loaders compare."""
from __future__ import annotations

import ctypes as C
import os
import re
import struct as _struct
from typing import Dict, List, Tuple

_INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")

_FIELD_CODES = {"int64_t": "q", "int32_t": "i", "uint32_t": "I", "uint64_t": "Q", "float": "f"}
_CTYPES = {"P": C.c_void_p, "q": C.c_int64, "i": C.c_int32, "I": C.c_uint32, "Q": C.c_uint64, "f": C.c_float}


class Header:
    """One parsed header: ``enums`` {enum name: enumerator names in order}, ``consts`` {name: int} of the enumerators and of every ``#define``
    that evaluates to an integer, ``structs`` {struct name: [(field, struct code)]} of every ``typedef struct``."""

    def __init__(self, file_name: str):
        self.path = os.path.join(_INCLUDE, file_name)
        with open(self.path) as f:
            self.text = re.sub(r"/\*.*?\*/|//[^\n]*", "", f.read(), flags=re.S)      # without its comments
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
        self.structs = {name: self._fields(body) for name, body in re.findall(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}", self.text, flags=re.S)}

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

    def exports(self, prefix: str) -> List[str]:
        """The functions the header declares whose names start with ``prefix``."""
        return re.findall(r"^\s*(?:int|void)\s+(%s\w+)\s*\(" % prefix, self.text, flags=re.M)

    def packer(self, name: str) -> _struct.Struct:
        return _struct.Struct("@" + "".join(code for _, code in self.structs[name]))      # native alignment: the C compiler's layout

    def ctypes_struct(self, name: str):
        def ctype(code):
            return _CTYPES[code[-1]] * int(code[:-1]) if len(code) > 1 else _CTYPES[code]
        return type(name, (C.Structure,), {"_fields_": [(f_, ctype(code)) for f_, code in self.structs[name]]})


SAMPLING = Header("diffspectra_hip.h")
TRAINING = Header("diffspectra_train.h")
