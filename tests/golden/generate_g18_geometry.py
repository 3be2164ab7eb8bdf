"""Generate ``g18_geometry.npz`` by running the REFERENCE's own ``evaluation/mmd.py`` and ``evaluation/cal_geometry.py``.

Runs only where the reference's source tree is present (``DIFFSPECTRA_REFERENCE``, as ``generate_golden.py``); never on the GPU box.
    python tests/golden/generate_g18_geometry.py
Two pins:
  MMD          the reference's ``compute_mmd`` on seeded fp32 inputs with ``batch_size`` 97 and 1000, and the same function on the same inputs
               widened to fp64 - inputs, both fp32 outputs and the fp64 output side by side;
  enumeration  the reference's ``get_bond_symbol``, ``get_bond_pairs`` / ``get_bond_pair_symbol`` and ``get_triple_bonds`` /
               ``get_triple_bond_symbol`` on small molecules given through a stand-in for the few RDKit ``Mol`` / ``Bond`` / ``Atom`` methods they
               call (the stand-in below is this project's code; ``rdkit`` itself is a stub in ``sys.modules`` and is never executed).
"""
from __future__ import annotations

import importlib
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("DIFFSPECTRA_REFERENCE", "/root/reference")
OUT = os.path.join(HERE, "g18_geometry.npz")
DECODER = ["H", "C", "N", "O", "F"]


# ---------------------------------------------------------------------------------------------- the RDKit stand-in
class Atom:
    def __init__(self, mol, idx, sym):
        self.mol, self.idx, self.sym = mol, idx, sym

    def GetSymbol(self):
        return self.sym

    def GetIdx(self):
        return self.idx

    def GetBonds(self):
        return [b for b in self.mol.bonds if self.idx in (b.begin, b.end)]


class Bond:
    def __init__(self, mol, idx, begin, end, order):
        self.mol, self.idx, self.begin, self.end, self.order = mol, idx, begin, end, order

    def GetIdx(self):
        return self.idx

    def GetBeginAtomIdx(self):
        return self.begin

    def GetEndAtomIdx(self):
        return self.end

    def GetBeginAtom(self):
        return self.mol.atoms[self.begin]

    def GetEndAtom(self):
        return self.mol.atoms[self.end]

    def GetBondType(self):
        return self.order                     # int(Chem.BondType.SINGLE | DOUBLE | TRIPLE) is 1 | 2 | 3


class Mol:
    def __init__(self, types, bonds):
        self.atoms = [Atom(self, i, DECODER[t]) for i, t in enumerate(types)]
        self.bonds = [Bond(self, k, b, e, o) for k, (b, e, o) in enumerate(bonds)]

    def GetBonds(self):
        return self.bonds

    def GetAtomWithIdx(self, i):
        return self.atoms[i]


def import_reference():
    for name in ("rdkit", "rdkit.Chem", "rdkit.Chem.rdMolTransforms"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["rdkit"].Chem = sys.modules["rdkit.Chem"]
    sys.modules["rdkit"].RDLogger = types.SimpleNamespace()
    for fn in ("GetBondLength", "GetAngleDeg", "GetDihedralDeg"):
        setattr(sys.modules["rdkit.Chem.rdMolTransforms"], fn, None)
    if "tqdm" not in sys.modules:
        try:
            import tqdm  # noqa: F401
        except ImportError:
            sys.modules["tqdm"] = types.SimpleNamespace(tqdm=lambda x, *a, **k: x)
    pkg = types.ModuleType("evaluation")
    pkg.__path__ = [os.path.join(REF, "evaluation")]      # package shell: submodules import, __init__ does not run
    sys.modules["evaluation"] = pkg
    mmd = importlib.import_module("evaluation.mmd")
    geo = importlib.import_module("evaluation.cal_geometry")
    assert mmd.__file__.startswith(REF) and geo.__file__.startswith(REF)
    return mmd, geo


# ---------------------------------------------------------------------------------------------- the molecules: (name, types, [(begin, end, order)])
def molecules():
    H, C, N, O = 0, 1, 2, 3
    return [
        ("ethane", [C, C, H, H, H, H, H, H], [(0, 1, 1), (0, 2, 1), (0, 3, 1), (4, 0, 1), (1, 5, 1), (6, 1, 1), (7, 1, 1)]),
        ("ethene", [C, C, H, H, H, H], [(0, 1, 2), (2, 0, 1), (0, 3, 1), (1, 4, 1), (5, 1, 1)]),
        ("propyne", [C, C, C, H, H, H, H], [(0, 1, 3), (1, 2, 1), (3, 0, 1), (2, 4, 1), (2, 5, 1), (6, 2, 1)]),
        ("cyclopropane", [C, C, C, H, H, H, H, H, H], [(0, 1, 1), (1, 2, 1), (2, 0, 1), (0, 3, 1), (4, 0, 1), (1, 5, 1), (6, 1, 1), (2, 7, 1), (8, 2, 1)]),
        ("methylhydrazine", [C, N, N, H, H, H, H, H, H], [(0, 1, 1), (2, 1, 1), (0, 3, 1), (0, 4, 1), (5, 0, 1), (1, 6, 1), (2, 7, 1), (8, 2, 1)]),
        ("dimethyl ether", [C, O, C, H, H, H, H, H, H], [(1, 0, 1), (1, 2, 1), (0, 3, 1), (4, 0, 1), (0, 5, 1), (2, 6, 1), (7, 2, 1), (2, 8, 1)]),
        ("acetaldehyde", [C, C, O, H, H, H, H], [(0, 1, 1), (1, 2, 2), (0, 3, 1), (4, 0, 1), (0, 5, 1), (6, 1, 1)]),
        ("ethanol", [C, C, O, H, H, H, H, H, H], [(1, 0, 1), (1, 2, 1), (3, 0, 1), (0, 4, 1), (0, 5, 1), (1, 6, 1), (7, 1, 1), (2, 8, 1)]),
        ("water and methane", [O, H, H, C, H, H, H, H], [(0, 1, 1), (2, 0, 1), (3, 4, 1), (5, 3, 1), (3, 6, 1), (7, 3, 1)]),
        ("lone atom", [C], []),
        ("butane skeleton", [C, C, C, C], [(1, 0, 1), (1, 2, 1), (3, 2, 1)]),
    ]


def enumeration(geo):
    out = []
    for name, types_, bonds in molecules():
        mol = Mol(types_, bonds)
        b_list = []
        for bond in mol.GetBonds():
            sym, rev = geo.get_bond_symbol(bond)
            b_list.append([sym, rev, [bond.GetBeginAtomIdx(), bond.GetEndAtomIdx()]])
        a_list = []
        for pair in geo.get_bond_pairs(mol):
            sym, ijk = geo.get_bond_pair_symbol(pair)
            rev, _ = geo.get_bond_pair_symbol(pair[::-1])
            a_list.append([sym, rev, [int(v) for v in ijk]])
        d_list = []
        for triple in geo.get_triple_bonds(mol):
            sym, ijkl = geo.get_triple_bond_symbol(triple)
            rev, _ = geo.get_triple_bond_symbol(triple[::-1])
            d_list.append([sym, rev, [int(v) for v in ijkl]])
        out.append(dict(name=name, types=types_, bonds=[list(b) for b in bonds], ref_bonds=b_list, ref_angles=a_list, ref_dihedrals=d_list))
    return out


# ---------------------------------------------------------------------------------------------- the MMD cases
def mmd_cases():
    rng = np.random.default_rng(20261118)
    f32 = lambda a: np.asarray(a, np.float32)
    cases = []
    sizes = [(2, 1), (1, 65), (63, 65), (300, 257), (513, 64), (700, 333), (1000, 1000)]
    for k, (ns, nt) in enumerate(sizes):
        if k % 3 == 0:        # bond lengths
            x, y = rng.normal(1.09, 0.02, ns), rng.normal(1.10, 0.03, nt)
        elif k % 3 == 1:      # bond angles
            x, y = rng.normal(109.5, 4.0, ns), rng.normal(111.0, 5.0, nt)
        else:                 # dihedrals
            x, y = rng.uniform(-180, 180, ns), np.concatenate([rng.normal(60, 15, nt // 2), rng.normal(-170, 20, nt - nt // 2)])
        cases.append((f"sizes_{ns}_{nt}", f32(x), f32(y)))
    cases.append(("constant_source", f32(np.full(40, 1.5)), f32(rng.normal(1.5, 0.05, 90))))
    cases.append(("all_identical", f32(np.full(7, 2.0)), f32(np.full(5, 2.0))))
    return cases


def main():
    mmd, geo = import_reference()
    arrays = {}
    names = []
    for name, x, y in mmd_cases():
        names.append(name)
        tx, ty = torch.tensor(x), torch.tensor(y)
        arrays[name + ".x"], arrays[name + ".y"] = x, y
        arrays[name + ".ref_b97"] = np.float64(mmd.compute_mmd(tx, ty, batch_size=97))
        arrays[name + ".ref_b1000"] = np.float64(mmd.compute_mmd(tx, ty, batch_size=1000))
        arrays[name + ".f64"] = np.float64(mmd.compute_mmd(tx.double(), ty.double(), batch_size=1000))
        print(name, arrays[name + ".ref_b97"], arrays[name + ".ref_b1000"], arrays[name + ".f64"])
    arrays["mmd_cases"] = np.array(json.dumps(names))
    arrays["enumeration"] = np.array(json.dumps(enumeration(geo)))
    np.savez_compressed(OUT, **arrays)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
