"""Generate ``g19_stability2d.npz`` by running the REFERENCE's own ``check_2D_stability`` (``evaluation/stability.py``) and ``eval_rdmol``
(``evaluation/rdkit_metric.py``) on small molecules.

Runs only where the reference's source tree is present (``DIFFSPECTRA_REFERENCE``, as ``generate_golden.py``); never on the GPU box.
    python tests/golden/generate_g19_stability2d.py
``rdkit`` is a stub in ``sys.modules`` and is never executed; the few ``Chem.RWMol`` / ``Atom`` / ``Conformer`` / ``Point3D`` / ``Kekulize`` /
``BondType`` methods the reference calls are the stand-in below, which is this project's code.  ``evaluation`` is a package shell, so its
``__init__`` does not run.  Two pins:
  stability    the reference's ``check_2D_stability`` with its own ``allowed_fc_bonds`` and the data set's ``atom_fc_num``
               (``datasets/datasets_config.py``): per molecule the inputs (types, charges, bond list), the reference's ``(molecule_stable,
               nr_stable_bonds, atom_num)`` and the formal charge it actually SET on every atom of the molecule it built.  This pins the
               stability table and the applied-charge rule against the reference's source.
  aggregation  the reference's ``eval_rdmol`` on the molecules ``check_2D_stability`` built, for several row lists with and without training
               molecules.  ``SanitizeMol``, ``GetMolFrags`` and ``MolToSmiles`` are the STAND-IN's there (the valence rule as this project
               restates RDKit's, components, a colour-refinement string), so this pins ONLY the aggregation - the denominators, the ``set``,
               the ``- {None}`` - and nothing about RDKit.
The list holds every (element, charge -2..+2) at a valence the reference allows and at one it does not, two fragments of equal size, an
isolated atom, a molecule valid but unstable (neutral N with one bond), one stable but invalid (OH3 with fc +1), and repeats under other
numberings for the uniqueness count.
"""
from __future__ import annotations

import importlib
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("DIFFSPECTRA_REFERENCE", "/root/reference")
OUT = os.path.join(HERE, "g19_stability2d.npz")
H, C, N, O, F = range(5)


# ---------------------------------------------------------------------------------------------- the RDKit stand-in
class BondType:
    SINGLE, DOUBLE, TRIPLE, AROMATIC = 1, 2, 3, 12


class Atom:
    def __init__(self, symbol):
        self.symbol, self.charge = symbol, 0

    def GetSymbol(self):
        return self.symbol

    def SetFormalCharge(self, charge):
        self.charge = int(charge)


class Bond:
    def __init__(self, begin, end, kind):
        self.begin, self.end, self.kind = begin, end, kind

    def GetBeginAtomIdx(self):
        return self.begin

    def GetEndAtomIdx(self):
        return self.end

    def GetBondType(self):
        return self.kind


class RWMol:
    def __init__(self):
        self.atoms, self.bonds, self.conformers = [], [], []

    def AddAtom(self, atom):
        self.atoms.append(atom)
        return len(self.atoms) - 1

    def AddBond(self, begin, end, kind):
        assert kind is not None and begin != end
        self.bonds.append(Bond(int(begin), int(end), kind))

    def AddConformer(self, conf):
        self.conformers.append(conf)

    def GetAtomWithIdx(self, i):
        return self.atoms[i]

    def GetAtoms(self):
        return self.atoms

    def GetBonds(self):
        return self.bonds

    def GetNumAtoms(self):
        return len(self.atoms)


class Conformer:
    def __init__(self, n):
        self.pos = [None] * n

    def SetAtomPosition(self, i, p):
        self.pos[i] = p


def Point3D(x, y, z):
    return (x, y, z)


# what stands for RDKit in eval_rdmol: this project's restated valence check, components, and a colour-refinement string as "SMILES"
VMAX = {("H", 0): 1, ("C", 0): 4, ("C", 1): 3, ("C", -1): 3, ("N", 0): 3, ("N", 1): 4, ("N", -1): 2, ("O", 0): 2, ("O", -1): 1, ("F", 0): 1}


def _valences(mol):
    val = [0] * len(mol.atoms)
    for b in mol.bonds:
        val[b.begin] += b.kind
        val[b.end] += b.kind
    return val


def SanitizeMol(mol):
    for atom, v in zip(mol.atoms, _valences(mol)):
        if v > VMAX[atom.symbol, atom.charge]:
            raise ValueError(f"valence {v} of {atom.symbol}{atom.charge:+d}")


def GetMolFrags(mol, asMols=True):
    n = len(mol.atoms)
    label = list(range(n))
    for _ in range(n):
        for b in mol.bonds:
            label[b.begin] = label[b.end] = min(label[b.begin], label[b.end])
    frags = []
    for root in sorted(set(label)):                       # by lowest atom
        members = [i for i in range(n) if label[i] == root]
        frag = RWMol()
        for i in members:
            a = Atom(mol.atoms[i].symbol)
            a.charge = mol.atoms[i].charge
            frag.AddAtom(a)
        for b in mol.bonds:
            if b.begin in members:
                frag.AddBond(members.index(b.begin), members.index(b.end), b.kind)
        frags.append(frag)
    return tuple(frags)


def MolToSmiles(mol):
    """Not a SMILES: the sorted colours of a colour refinement over (element, charge, bond orders), hashed so that they compare across
    molecules.  It tells the molecules of this list apart exactly when their labelled graphs differ (checked in main against the
    backtracking comparison of tests/graph_mirror.py)."""
    import hashlib
    colour = [f"{a.symbol}{a.charge:+d}" for a in mol.atoms]
    nbrs = [[] for _ in mol.atoms]
    for b in mol.bonds:
        nbrs[b.begin].append((b.end, b.kind))
        nbrs[b.end].append((b.begin, b.kind))
    for _ in range(len(mol.atoms)):
        colour = [hashlib.md5(repr((c, sorted((k, colour[j]) for j, k in nbrs[i]))).encode()).hexdigest()[:16] for i, c in enumerate(colour)]
    return ".".join(sorted(colour))


def import_reference():
    for name in ("rdkit", "rdkit.Chem", "rdkit.Chem.rdchem", "rdkit.Chem.rdmolops", "rdkit.Geometry"):
        sys.modules[name] = types.ModuleType(name)
    chem = sys.modules["rdkit.Chem"]
    sys.modules["rdkit"].Chem = chem
    chem.rdchem, chem.rdmolops = sys.modules["rdkit.Chem.rdchem"], sys.modules["rdkit.Chem.rdmolops"]
    chem.rdchem.BondType = BondType
    chem.rdmolops.GetMolFrags = GetMolFrags
    chem.RWMol, chem.Atom, chem.Conformer = RWMol, Atom, Conformer
    chem.Kekulize = lambda mol: None                      # the records hold no aromatic bonds
    chem.SanitizeMol, chem.MolToSmiles = SanitizeMol, MolToSmiles
    chem.AllChem = chem.QED = chem.Descriptors = None     # imported by rdkit_metric.py, not used by eval_rdmol
    sys.modules["rdkit.Geometry"].Point3D = Point3D
    pkg = types.ModuleType("evaluation")
    pkg.__path__ = [os.path.join(REF, "evaluation")]      # package shell: submodules import, __init__ does not run
    sys.modules["evaluation"] = pkg
    stability = importlib.import_module("evaluation.stability")
    metric = importlib.import_module("evaluation.rdkit_metric")
    spec = importlib.util.spec_from_file_location("ref_datasets_config", os.path.join(REF, "datasets", "datasets_config.py"))
    config = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(config)
    assert stability.__file__.startswith(REF) and metric.__file__.startswith(REF)
    return stability, metric, config.qm9_with_h


# ---------------------------------------------------------------------------------------------- the molecules: (name, types, charges, [(i, j, order)])
def star(centre, charge, k, name=None):
    """``centre`` with ``k`` hydrogens on single bonds."""
    return (name or f"{'HCNOF'[centre]}{charge:+d} with {k} H", [centre] + [H] * k, [charge] + [0] * k, [(0, i + 1, 1) for i in range(k)])


def molecules(allowed_fc_bonds):
    out = []
    for t, sym in enumerate("HCNOF"):
        table = allowed_fc_bonds[sym]
        for charge in (-2, -1, 0, 1, 2):
            allowed = table[charge] if charge in table else table[0]
            allowed = [allowed] if isinstance(allowed, int) else list(allowed)
            out.append(star(t, charge, allowed[0]))
            out.append(star(t, charge, min(v for v in range(6) if v not in allowed)))
    out += [
        star(C, 0, 4, "CH4"), star(N, 1, 4, "NH4 fc +1"), star(O, 1, 3, "OH3 fc +1 (stable, invalid)"), star(N, 0, 1, "NH (valid, unstable)"),
        ("CH3 fc +2 and an H fc +1", [C, H, H, H, H], [2, 0, 0, 0, 1], [(0, 1, 1), (0, 2, 1), (0, 3, 1)]),
        ("F fc -1 beside H fc +1", [F, H], [-1, 1], []),
        ("CH4 renumbered", [H, H, C, H, H], [0] * 5, [(2, 0, 1), (1, 2, 1), (2, 3, 1), (4, 2, 1)]),
        ("water", [O, H, H], [0] * 3, [(0, 1, 1), (0, 2, 1)]),
        ("water renumbered", [H, O, H], [0] * 3, [(0, 1, 1), (2, 1, 1)]),
        ("two waters (equal fragments)", [H, O, H, O, H, H], [0] * 6, [(0, 1, 1), (1, 2, 1), (3, 4, 1), (3, 5, 1)]),
        ("water and methane", [O, H, H, C, H, H, H, H], [0] * 8, [(0, 1, 1), (2, 0, 1), (3, 4, 1), (5, 3, 1), (3, 6, 1), (7, 3, 1)]),
        ("methane and water", [C, H, H, H, H, O, H, H], [0] * 8, [(0, 1, 1), (0, 2, 1), (0, 3, 1), (0, 4, 1), (5, 6, 1), (5, 7, 1)]),
        ("water and a lone carbon", [C, O, H, H], [0] * 4, [(1, 2, 1), (1, 3, 1)]),
        ("lone carbon", [C], [0], []),
        ("carbon dioxide", [O, C, O], [0] * 3, [(0, 1, 2), (1, 2, 2)]),
        ("hydrogen cyanide", [H, C, N], [0] * 3, [(0, 1, 1), (1, 2, 3)]),
        ("dinitrogen", [N, N], [0] * 2, [(0, 1, 3)]),
        ("formaldehyde", [C, O, H, H], [0] * 4, [(0, 1, 2), (0, 2, 1), (0, 3, 1)]),
        ("ethanol", [C, C, O, H, H, H, H, H, H], [0] * 9, [(1, 0, 1), (1, 2, 1), (3, 0, 1), (0, 4, 1), (0, 5, 1), (1, 6, 1), (7, 1, 1), (2, 8, 1)]),
        ("dimethyl ether", [C, O, C, H, H, H, H, H, H], [0] * 9, [(1, 0, 1), (1, 2, 1), (0, 3, 1), (4, 0, 1), (0, 5, 1), (2, 6, 1), (7, 2, 1), (2, 8, 1)]),
        ("nitromethane, charges separated", [C, N, O, O, H, H, H], [0, 1, 0, -1, 0, 0, 0], [(0, 1, 1), (1, 2, 2), (1, 3, 1), (0, 4, 1), (0, 5, 1), (0, 6, 1)]),
        ("five-valent carbon", [C, H, H, H, H, H], [0] * 6, [(0, k, 1) for k in range(1, 6)]),
        ("carbon with a double and three single bonds", [C, O, H, H, H], [0] * 5, [(0, 1, 2), (0, 2, 1), (0, 3, 1), (0, 4, 1)]),
    ]
    return out


def run(stability, info, mol):
    name, types_, charges, bonds = mol
    n = len(types_)
    edge = torch.zeros(n, n, dtype=torch.long)
    for i, j, order in bonds:
        edge[i, j] = edge[j, i] = order
    pos = torch.zeros(n, 3)
    stable, nr_stable, atom_num, rdmol = stability.check_2D_stability(pos, torch.tensor(types_), torch.tensor(charges), edge, info)
    row = dict(name=name, types=types_, charges=charges, bonds=[list(b) for b in bonds], ref_stable=bool(stable), ref_nr_stable=int(nr_stable),
               ref_atom_num=int(atom_num), ref_applied=[a.charge for a in rdmol.GetAtoms()])
    return row, rdmol


def _same_graph(a, b):
    """The check behind MolToSmiles' docstring: exact identity of the labelled graphs (tests/graph_mirror.py)."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from tests import graph_mirror as GM
    as_dict = lambda m: GM.molecule(["HCNOF".index(x.symbol) for x in m.atoms], [(x.begin, x.end) for x in m.bonds], fc=[x.charge for x in m.atoms],
                                    orders=[x.kind for x in m.bonds])
    return GM.same_graph(as_dict(a), as_dict(b))


def main():
    stability, metric, info = import_reference()
    from evaluation.bond_analyze import allowed_fc_bonds
    rows, rdmols = zip(*(run(stability, info, mol) for mol in molecules(allowed_fc_bonds)))
    for row in rows:
        print(f"{row['name']:45s} stable atoms {row['ref_nr_stable']}/{row['ref_atom_num']}  charges set {row['ref_applied']}")
    # the stand-in's string separates exactly the distinct graphs among everything eval_rdmol will ask it about
    asked = [f for m in rdmols for f in GetMolFrags(m)] + list(rdmols)
    for a in asked:
        for b in asked:
            assert (MolToSmiles(a) == MolToSmiles(b)) == _same_graph(a, b)
    index = {row["name"]: k for k, row in enumerate(rows)}
    everything = list(range(len(rows)))
    known = [index[k] for k in ("water", "carbon dioxide", "ethanol", "OH3 fc +1 (stable, invalid)", "lone carbon")]
    lists = [("all", everything, None), ("all, with known", everything, known), ("nothing valid", [index["OH3 fc +1 (stable, invalid)"], index["five-valent carbon"]], known),
             ("fragments", [index[k] for k in ("two waters (equal fragments)", "water and methane", "methane and water", "water", "CH4", "water and a lone carbon")], known[:1]),
             ("one row", [index["CH4"]], None)]
    cases = []
    for name, take, train in lists:
        train_smiles = None if train is None else [MolToSmiles(rdmols[k]) for k in train]       # get_2D_edm_metric: MolToSmiles of train_mols
        result = metric.eval_rdmol([rdmols[k] for k in take], train_smiles)
        cases.append(dict(name=name, rows=take, known=train, result={k: float(v) for k, v in result.items()}))
        print(name, result)
    np.savez_compressed(OUT, molecules=np.array(json.dumps(list(rows))), eval_rdmol=np.array(json.dumps(cases)),
                        atom_fc_num=np.array(json.dumps(sorted(info["atom_fc_num"]))))
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(rows), "molecules")


if __name__ == "__main__":
    main()
