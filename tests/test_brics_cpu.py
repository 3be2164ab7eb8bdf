"""CPU: the C-ABI surface of the BRICS analytics (include/diffspectra_brics.h) and its argument checks (fake pointers: nothing that would pass
every check is ever passed), the bindings' refusals, and the mirror of tests/brics_mirror.py on the hand-stated table of molecules - the pin of
the definitions, since RDKit cannot run here - under renumbering, with the header's invariants, and on the derived set whose coverage the GPU
comparison relies on.  (The kernels are checked on the GPU against the same mirror: tests/test_brics_gpu.py.)"""
import ctypes as C
import math
import re

import numpy as np
import pytest
import torch

from diffspectra_amd import abi, engine as E, structure_metrics as S
from tests import brics_mirror as B, graph_mirror as GM, structure_mirror as SM
from tests.test_scaffold_cpu import MirrorEngine as GraphMirrorEngine, same_partition

OK, ERR_ARG = 0, -1
FAKE = 0x1000                        # a 16-byte aligned address that is nobody's memory


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return E.load_library()


@pytest.fixture(scope="module")
def table():
    """The hand-stated molecules with their records and the mirror's rows, computed once."""
    rows = B.hand_table()
    rec, n = SM.records([mol for _, mol, _ in rows])
    return rows, rec, n, B.analyse_table(rec, n)


@pytest.fixture(scope="module")
def derived():
    mols = B.derived_set()
    rec, n = SM.records(mols)
    return mols, rec, n, [B.Analysis(r, k) for r, k in zip(rec, n)]


# ------------------------------------------------------------------------------------------------------------------ the C-ABI surface

RECORDS = (["rec", "n", "P", "env", "cuts", "fragment_of", "summary", "status", "stream"], ["*", "*", "int64_t", "*", "*", "*", "*", "*", "*"])
FRAGMENTS = (["rec", "n", "P", "first", "F", "aromatic", "out_rec", "out_n", "out_owner", "out_source", "stream"],
             ["*", "*", "int64_t", "*", "int64_t", "int32_t", "*", "*", "*", "*", "*"])


def test_header_declares_and_library_exports_the_brics_functions(lib):
    assert abi.BRICS.exports("dsb_") == list(abi.BRICS.prototypes) == ["dsb_brics_records", "dsb_brics_fragment_records"]
    hdr = re.sub(r"/\*.*?\*/", "", open(abi.BRICS.path).read(), flags=re.S)
    for name, (names, kinds) in (("dsb_brics_records", RECORDS), ("dsb_brics_fragment_records", FRAGMENTS)):
        assert hasattr(lib, name)
        args = re.search(r"int\s+" + name + r"\s*\((.*?)\)\s*;", hdr, flags=re.S).group(1)
        assert [a.split()[-1].lstrip("*") for a in args.split(",")] == names
        proto = abi.BRICS.prototypes[name]
        assert proto.params == list(zip(names, kinds)) and proto.ret == "int"
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == proto.argtypes                                      # bound from the header
    consts = abi.BRICS.consts
    assert (consts["DSB_OK"], consts["DSB_UNUSABLE"], consts["DSB_MAX_CUTS"], consts["DSB_ATTACH_TYPE"], consts["DSB_AROMATIC_ORDER"]) == (0, 3, 28, 5, 4)
    assert 1 <= consts["DSB_WAVES"] <= 16 and consts["DSB_NUM_RULES"] == len(S.BRICS_RULES) == 40
    assert (E.BRICS_OK, E.BRICS_UNUSABLE) == (0, 3) == (B.OK, B.UNUSABLE) and E.BRICS_CONSTS is consts
    assert (E.BRICS_MAX_CUTS, E.BRICS_ATTACH_TYPE, E.BRICS_AROMATIC_ORDER) == (B.MAX_CUTS, B.ATTACH_TYPE, B.AROMATIC_ORDER)
    for other in (abi.SAMPLING, abi.TRAINING, abi.SETS, abi.VALENCE, abi.GROUPS, abi.SCAFFOLD, abi.SMILES, abi.SUBSTRUCTURE, abi.STEREO, abi.TILES):
        assert not other.exports("dsb_")


def test_library_without_the_symbols_is_refused(lib):
    class Hollow:
        def __getattr__(self, name):
            if name.startswith("dsb_"):
                raise AttributeError(name)
            return getattr(lib, name)
    with pytest.raises(AttributeError, match="dsb_"):
        abi.BRICS.bind(Hollow())


def test_rules_and_labels_are_the_headers():
    """``BRICS_RULES`` and the mirror's table equal the rules parsed from the header's text, in its order; so do the labels."""
    text = open(abi.BRICS.path).read()
    block = text[text.index("BRICS-RULES-BEGIN") + len("BRICS-RULES-BEGIN"):text.index("BRICS-RULES-END")]
    parsed = [(int(x), int(y), 2 if sign == "=" else 1) for x, sign, y in re.findall(r"(\d+)([-=])(\d+)", block)]
    assert parsed == list(S.BRICS_RULES) == B.RULES and len(parsed) == abi.BRICS.consts["DSB_NUM_RULES"] and len(set(parsed)) == 40
    labels = tuple(int(x) for x in re.search(r"DSB_LABELS = ([\d ]+)\.", text).group(1).split())
    assert labels == S.BRICS_LABELS == B.LABELS and {e for x, y, _ in parsed for e in (x, y)} == set(labels) and len(labels) == 13
    assert [int(x) for x in re.findall(r"^ \*   L(\d+) ", text, flags=re.M)] == list(labels)                 # one environment line per label
    assert [r for r in parsed if r[2] == 2] == [(7, 7, 2)] and not {11, 12} & set(labels)
    for word in ("UNPINNED", "13-15", "fragments = components of the matchable graph + cuts", "two bridges", "4-11, 5-12, 11-13, 11-14, 11-15, 11-16"):
        assert word in text, word


def _records(lib, P=1, rec=FAKE, n=FAKE, outputs=None):
    return lib.dsb_brics_records(rec, n, P, *([FAKE] * 5 if outputs is None else outputs), None)


def _fragments(lib, P=1, rec=FAKE, n=FAKE, first=FAKE, F=4, aromatic=1, outputs=None):
    return lib.dsb_brics_fragment_records(rec, n, P, first, F, aromatic, *([FAKE] * 4 if outputs is None else outputs), None)


def test_empty_calls_launch_nothing(lib):
    assert _records(lib, P=0, rec=None, n=None, outputs=[None] * 5) == OK and _records(lib, P=0, rec=FAKE + 1) == OK
    assert _fragments(lib, P=0, rec=None, n=None, first=None, outputs=[None] * 4) == OK and _fragments(lib, P=0, rec=FAKE + 1, outputs=[FAKE + 2] + [FAKE] * 3) == OK
    assert _fragments(lib, P=0, F=0) == OK


def test_argument_errors_in_the_stated_order(lib):
    """Every pointer here is fake or NULL: a call that got past its checks would fault, so each line also shows that the check comes first."""
    for P in (-1, 2 ** 31, -2 ** 40):                                           # the size, before "an empty call launches nothing" and before any pointer
        assert _records(lib, P=P) == ERR_ARG and _records(lib, P=P, rec=None, n=None, outputs=[None] * 5) == ERR_ARG
        assert _fragments(lib, P=P) == ERR_ARG and _fragments(lib, P=P, rec=None, n=None, first=None, outputs=[None] * 4) == ERR_ARG
    for aromatic, F in ((2, 4), (-1, 4), (1, -1), (0, -2 ** 40)):               # the scalars, also before P = 0
        assert _fragments(lib, aromatic=aromatic, F=F) == ERR_ARG and _fragments(lib, P=0, aromatic=aromatic, F=F, rec=None, n=None, first=None, outputs=[None] * 4) == ERR_ARG
    assert _records(lib, rec=None) == ERR_ARG and _records(lib, n=None) == ERR_ARG
    assert _fragments(lib, rec=None) == ERR_ARG and _fragments(lib, n=None) == ERR_ARG and _fragments(lib, first=None) == ERR_ARG
    for off in (1, 2, 3):
        assert _records(lib, rec=FAKE + off) == ERR_ARG and _fragments(lib, rec=FAKE + off) == ERR_ARG
        assert _fragments(lib, outputs=[FAKE + off] + [FAKE] * 3) == ERR_ARG
    for k in range(5):
        out = [FAKE] * 5
        out[k] = None
        assert _records(lib, outputs=out) == ERR_ARG, f"output {k}"
    for k in range(4):
        out = [FAKE] * 4
        out[k] = None
        assert _fragments(lib, outputs=out) == ERR_ARG, f"output {k}"


def test_bindings_refuse_wrong_arguments():
    """Arguments are checked, never converted; and there is no CPU path."""
    rec, n = torch.zeros(4, E.RECORD_BYTES, dtype=torch.uint8), torch.full((4,), 3, dtype=torch.int32)
    first = torch.arange(4, dtype=torch.int64)
    for records in (E.brics_records, E.DmtEngine.brics_records.__get__(object())):
        with pytest.raises(TypeError, match="rec"):
            records(rec.int(), n)
        with pytest.raises(TypeError, match="n must"):
            records(rec, n.long())
        with pytest.raises(ValueError, match="rec"):
            records(rec[:, :1000].contiguous(), n)
        with pytest.raises(ValueError, match="n must"):
            records(rec, n[:3])
        with pytest.raises(ValueError, match="contiguous"):
            records(torch.zeros(E.RECORD_BYTES, 4, dtype=torch.uint8).t(), n)
        with pytest.raises(TypeError, match="tensor"):
            records(rec.numpy(), n)
        with pytest.raises(RuntimeError, match="no CPU path"):
            records(rec, n)
    for fragments in (E.brics_fragment_records, E.DmtEngine.brics_fragment_records.__get__(object())):
        with pytest.raises(TypeError, match="rec"):
            fragments(rec.int(), n, first, 4)
        with pytest.raises(TypeError, match="first must"):
            fragments(rec, n, first.int(), 4)
        with pytest.raises(ValueError, match="first must"):
            fragments(rec, n, first[:3], 4)
        with pytest.raises(TypeError, match="aromatic"):
            fragments(rec, n, first, 4, 1)
        with pytest.raises(TypeError, match="rows"):
            fragments(rec, n, first, 4.0)
        with pytest.raises(TypeError, match="rows"):
            fragments(rec, n, first, True)
        with pytest.raises(ValueError, match="rows"):
            fragments(rec, n, first, -1)
        with pytest.raises(RuntimeError, match="no CPU path"):
            fragments(rec, n, first, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        S.brics(rec, n)
    with pytest.raises(RuntimeError, match="no CPU path"):
        S.brics_fragment_records(rec, n)
    with pytest.raises(RuntimeError, match="no CPU path"):
        S.get_fragment_metric((rec, n), unique=False)


# ------------------------------------------------------------------------------------------------------------------ the mirror, pinned by hand

def test_mirror_on_the_hand_stated_table(table):
    rows, rec, n, got = table
    assert len(rows) >= 24 and len({name for name, *_ in rows}) == len(rows)
    for (name, mol, cuts), g in zip(rows, got):
        assert g["cuts"] == sorted(cuts) and g["status"] == B.OK and g["summary"][1] == len(cuts), (name, g["cuts"])
        assert all(a < b for a, b, _, _ in cuts)
    seen = {label for _, _, cuts in rows for _, _, la, lb in cuts for label in (la, lb)}
    assert seen == set(B.LABELS)                                                # every label occurs as a cut label in the table
    by_name = {name: k for k, (name, *_) in enumerate(rows)}
    env = lambda name, atom: {e for e in range(32) if (got[by_name[name]]["env"][atom] >> e) & 1}
    # the environments behind some of the anchors
    assert env("CCNOC", 2) == set() and env("CCNOC", 3) == {3} and env("CC=NCC", 2) == set() and env("CC=NCC", 1) == {7}
    assert env("N-methylacetamide", 1) == {1, 6, 7} and env("N-methylacetamide", 3) == {5} and env("N-methylacetamide", 4) == set()
    assert env("1-ethylpyrrolidin-2-one", 0) == {10} and env("1-ethylpyrrolidin-2-one", 1) == {1, 7, 13}    # the lactam N is not L5
    assert env("1-methoxy-7-oxabicyclo[2.2.1]heptane", 0) == {13, 15} and env("1-methoxy-7-oxabicyclo[2.2.1]heptane", 6) == set()
    assert env("1,1'-bi(2-oxabicyclo[1.1.0]butyl)", 0) == env("1,1'-bi(2-oxabicyclo[1.1.0]butyl)", 4) == {4, 13, 15}
    assert env("2-ethylpyridine", 0) == {9} and env("2-ethylpyridine", 1) == {14} and env("2-ethylpyridine", 3) == {16}
    assert env("ethanol whose hydroxyl hydrogen bridges to ethyl", 2) == {3} and env("ethanol whose hydroxyl hydrogen bridges to ethyl", 3) == set()
    assert got[by_name["ethanol whose hydroxyl hydrogen bridges to ethyl"]]["summary"] == (6, 1, 2, 9)      # the bridging hydrogen is matchable
    two = got[by_name["N-methylacetamide and but-2-ene"]]
    assert two["summary"] == (9, 2, 4, 6) and two["fragment_of"][:9] == [0, 0, 0, 1, 1, 2, 2, 3, 3]
    # the fragments of ethyl acetate: acetyl with [1*], the bridging O with [3*] twice, ethyl with [4*]
    k = by_name["ethyl acetate"]
    frags = B.fragment_rows(rec[k], n[k])
    assert [m for _, m, _ in frags] == [3 + 3 + 1, 1 + 2, 2 + 5 + 1] and frags[0][2][:7] == [0, 1, 2, 6, 7, 8, 3] and frags[1][2][:3] == [3, 1, 4]
    o = SM.mol_from_record(frags[1][0], frags[1][1])
    assert o["type"].tolist() == [3, 5, 5] and o["fc"].tolist() == [0, 3, 3] and o["bond"].tolist() == [[0, 1, 1], [1, 0, 0], [1, 0, 0]]
    acetyl = SM.mol_from_record(frags[0][0], frags[0][1])
    assert acetyl["type"].tolist() == [1, 1, 3, 0, 0, 0, 5] and acetyl["fc"].tolist()[-1] == 1 and acetyl["bond"][1].tolist() == [1, 0, 2, 0, 0, 0, 1]
    assert np.array_equal(acetyl["pos"][6], SM.mol_from_record(rec[k], n[k])["pos"][3])                     # the attachment sits where the oxygen was


def test_table_under_renumbering(table):
    """Cuts, labels and fragment classes do not depend on the atom numbering - the both-orientations case included."""
    rows, rec, n, got = table
    rng = np.random.default_rng(17)
    for (name, mol, cuts), r, k, g in zip(rows, rec, n, got):
        mine = [B.fragment_mols(r, k, aromatic) for aromatic in (True, False)]
        for _ in range(3):
            perm = rng.permutation(len(mol["type"]))
            (r2,), (k2,) = SM.records([B.renumbered(mol, perm)])
            h = B.analyse(r2, k2)
            assert h["cuts"] == B.moved_cuts(cuts, perm) and h["summary"] == g["summary"], name
            for aromatic, want in zip((True, False), mine):
                theirs = B.fragment_mols(r2, k2, aromatic)
                assert len(theirs) == len(want) and same_multiset(theirs, want), (name, aromatic)


def same_multiset(a, b):
    """Two lists of molecules hold the same graphs the same number of times."""
    left = list(b)
    for mol in a:
        for k, other in enumerate(left):
            if GM.same_graph(mol, other):
                del left[k]
                break
        else:
            return False
    return not left


def test_invariants_on_every_record(table, derived):
    """fragments = components + cuts; a fragment's atoms plus its attachment points are at most n; every cut is a chain bond whose other
    ends are distinct atoms outside the fragment."""
    rows, rec, n, _ = table
    mols, d_rec, d_n, found = derived
    for r, k, A in list(zip(rec, n, [B.Analysis(r, k) for r, k in zip(rec, n)])) + list(zip(d_rec, d_n, found)):
        assert A.usable and len(A.fragments) == len(A.components) + len(A.cuts)
        assert sorted(a for f in A.fragments for a in f) == list(range(int(k)))                            # every atom in exactly one fragment
        for out, m, source in B.fragment_rows(r, k, True, A):
            assert m <= int(k) <= 29 and len(set(source[:m])) == m and source[m:] == [0xff] * (29 - m)
        assert all(not A.ring[a, b] for a, b, _, _ in A.cuts)


def test_mirror_on_unusable_and_malformed_records(table):
    rows, rec, n, got = table
    zero = dict(env=[0] * 29, cuts=[], fragment_of=[0xff] * 29, summary=(0, 0, 0, 0), status=B.UNUSABLE)
    k = [name for name, *_ in rows].index("ethyl acetate")
    base, count = rec[k], int(n[k])
    assert B.analyse(base, 0) == zero and B.analyse(base, -2) == zero and B.fragment_rows(base, 0) == []
    bad = base.copy()
    bad[SM.TYPE + 3] = 5
    assert B.analyse(bad, count) == zero
    bad = base.copy()
    bad[SM.BOND + 2 * 29 + 9] = 4
    assert B.analyse(bad, count) == zero
    fine = base.copy()                                                          # the lower triangle, the diagonal, atoms >= n and the pad are not looked at
    fine[SM.BOND + 9 * 29 + 2] = fine[SM.BOND + 4 * 29 + 4] = fine[SM.TYPE + count] = fine[SM.FC + count + 1] = fine[SM.BOND + 1 * 29 + count] = 200
    fine[SM.BOND_END:] = 0xEE
    assert B.analyse(fine, count) == got[k]
    assert all(np.array_equal(a[0], b[0]) and a[1:] == b[1:] for a, b in zip(B.fragment_rows(fine, count), B.fragment_rows(base, count)))
    env, cuts, fragment_of, summary, status = B.as_arrays([got[k], zero])
    assert cuts.shape == (2, 28, 4) and cuts[0, :2].tolist() == [[1, 3, 1, 3], [3, 4, 3, 4]] and (cuts[0, 2:] == 0xff).all() and (cuts[1] == 0xff).all()
    assert (fragment_of[1] == 0xff).all() and not env[1].any() and status.tolist() == [0, 3]
    dense = B.analyse(*[x[0] for x in SM.records([GM.k29()])])
    assert dense["summary"] == (29, 0, 1, 29) and dense["cuts"] == []


def kekule_differs(found, rec, n):
    """The records with a fragment whose aromatic-byte class holds fragments of several Kekule classes, over the whole set."""
    aromatic, kekule, seen = B.Classes(), B.Classes(), []
    for p, (r, k, A) in enumerate(zip(rec, n, found)):
        with_byte, with_orders = B.fragment_rows(r, k, True, A), B.fragment_rows(r, k, False, A)
        for (a, m, _), (b, _, _) in zip(with_byte, with_orders):
            seen.append((p, aromatic.find(SM.mol_from_record(a, m)), kekule.find(SM.mol_from_record(b, m))))
    drawings = {}
    for _, a, b in seen:
        drawings.setdefault(a, set()).add(b)
    return sorted({p for p, a, _ in seen if len(drawings[a]) > 1})


def test_derived_set_covers_the_ground_the_gpu_comparison_stands_on(derived):
    mols, rec, n, found = derived
    assert 250 <= len(mols) <= 350 and max(len(m["type"]) for m in mols) <= 29
    got = [B.analyse(r, k, A) for r, k, A in zip(rec, n, found)]
    assert all(g["status"] == B.OK for g in got)
    assert sum(g["summary"][1] == 0 for g in got) >= 40 and sum(g["summary"][1] >= 2 for g in got) >= 40
    ends = [label for g in got for _, _, la, lb in g["cuts"] for label in (la, lb)]
    assert all(ends.count(label) >= 5 for label in B.LABELS), {label: ends.count(label) for label in B.LABELS}
    assert len(kekule_differs(found, rec, n)) >= 10
    assert all(np.array_equal(a["bond"], b["bond"]) and np.array_equal(a["type"], b["type"]) for a, b in zip(mols, B.derived_set()))      # fixed by the seed


def test_kekule_drawings_are_one_fragment_with_the_aromatic_byte():
    for name, a, b in B.kekule_pairs():
        (ra, rb), (na, nb) = SM.records([a, b])
        assert B.analyse(ra, na) == B.analyse(rb, nb) and B.analyse(ra, na)["summary"][1] >= 1, name
        assert same_multiset(B.fragment_mols(ra, na, True), B.fragment_mols(rb, nb, True)), name
        assert not same_multiset(B.fragment_mols(ra, na, False), B.fragment_mols(rb, nb, False)), name


def test_frag_of_the_mirror(table):
    assert B.cosine({"A": 2, "B": 1}, {"A": 2, "B": 1}) == 1.0 and B.cosine({"A": 3}, {"A": 7}) == 1.0
    assert B.cosine({"A": 2, "B": 1}, {"C": 1, "D": 5}) == 0.0
    assert B.cosine({"A": 2, "B": 1}, {"A": 1, "C": 2}) == 2 / math.sqrt(5 * 5) == 0.4
    assert math.isnan(B.cosine({}, {"A": 1})) and math.isnan(B.cosine({"A": 1}, {})) and math.isnan(B.cosine({}, {}))
    # the same on records.  Fragments: methyl acetate = acetyl[1*] + [3*]O-CH3; ethyl acetate = acetyl[1*] + [3*]O[3*] + ethyl[4*];
    # N-ethylacetamide = acetyl[1*] + [5*]NH[5*] + ethyl[4*]; ethanol = itself
    rows, rec, n, got = table
    names = [name for name, *_ in rows]
    pick = lambda *ns: (rec[[names.index(x) for x in ns]], n[[names.index(x) for x in ns]])
    gen, test = pick("methyl acetate", "ethyl acetate", "ethanol"), pick("N-ethylacetamide", "ethyl acetate", "ethyl acetate")
    # generated: acetyl 2, OMe 1, O 1, ethyl 1, ethanol 1; test: acetyl 3, NH 1, ethyl 3, O 2
    assert B.fragment_metric(gen, test)["frag"] == (2 * 3 + 1 * 2 + 1 * 3) / math.sqrt((4 + 1 + 1 + 1 + 1) * (9 + 1 + 9 + 4))
    full = B.fragment_metric(gen, test)
    assert (full["fragments_generated"], full["fragments_test"], full["distinct_generated"], full["distinct_test"], full["shared"]) == (6, 9, 5, 4, 3)
    assert full["owner"] == [0, 0, 1, 1, 1, 2] and full["mean_cuts"] == (1 + 2 + 0) / 3 and (full["n_generated"], full["n_test"]) == (3, 3)
    assert B.fragment_metric(gen, gen)["frag"] == 1.0 and B.fragment_metric(pick("ethanol"), pick("toluene"))["frag"] == 0.0
    empty = (rec[:0], n[:0])
    assert math.isnan(B.fragment_metric(empty, test)["frag"]) and math.isnan(B.fragment_metric(gen, empty)["frag"]) and math.isnan(B.fragment_metric(empty, test)["mean_cuts"])


# ------------------------------------------------------------------------------------------------------------------ host arithmetic

class MirrorEngine(GraphMirrorEngine):
    """An engine that answers from the mirrors: what ``structure_metrics`` does around the kernels, without them."""

    def brics_records(self, rec, n):
        return tuple(torch.from_numpy(a) for a in B.as_arrays(B.analyse_table(rec.numpy(), n.numpy())))

    def brics_fragment_records(self, rec, n, first, rows, aromatic=True):
        out = (torch.zeros(rows, E.RECORD_BYTES, dtype=torch.uint8), torch.zeros(rows, dtype=torch.int32), torch.zeros(rows, dtype=torch.int64),
               torch.full((rows, 29), 0xff, dtype=torch.uint8))
        for p, (r, k) in enumerate(zip(rec.numpy(), n.numpy())):
            for f, (row, m, source) in enumerate(B.fragment_rows(r, k, aromatic)):
                at = int(first[p]) + f
                if 0 <= at < rows:
                    out[0][at], out[1][at], out[2][at], out[3][at] = torch.from_numpy(row), int(m), p, torch.tensor(source, dtype=torch.uint8)
        return out


def test_public_interface_on_the_mirror_engine(table, derived):
    rows, rec, n, got = table
    eng = MirrorEngine()
    t_rec, t_n = torch.from_numpy(rec), torch.from_numpy(n)
    found = S.brics(t_rec, t_n.tolist(), engine=eng)
    assert isinstance(found, S.Brics) and found.usable.all() and found.n_cuts.tolist() == [len(c) for _, _, c in rows]
    assert found.n_fragments.tolist() == [g["summary"][2] for g in got] and found.env.shape == (len(rows), 29) and found.cuts.shape == (len(rows), 28, 4)
    for aromatic in (True, False):
        f_rec, f_n, owner, source = S.brics_fragment_records(t_rec, t_n, aromatic=aromatic, engine=eng)
        want = B.fragment_table(rec, n, aromatic)
        assert f_rec.dtype == torch.uint8 and f_n.dtype == torch.int32 and owner.dtype == torch.int64 and source.dtype == torch.uint8
        assert all(np.array_equal(a.numpy(), b) for a, b in zip((f_rec, f_n, owner, source), want)) and f_rec.shape[0] == int(found.n_fragments.sum())
    assert [t.shape[0] for t in S.brics_fragment_records(t_rec[:0], t_n[:0], engine=eng)] == [0] * 4
    # the set metric against the mirror, with and without the molecules made unique, with a keep mask, with Kekule orders
    mols, d_rec, d_n, _ = derived
    gen, test = (d_rec[30:200:3], d_n[30:200:3]), (np.concatenate([d_rec[31:200:3], d_rec[30:60:3]]), np.concatenate([d_n[31:200:3], d_n[30:60:3]]))
    for aromatic in (True, False):
        want = B.fragment_metric(gen, test, aromatic)
        assert 0.0 < want["frag"] < 1.0 and want["shared"] >= 3
        fn = S.get_fragment_metric((torch.from_numpy(test[0]), test[1]), unique=False, aromatic=aromatic, engine=eng)
        mine = fn((torch.from_numpy(gen[0]), gen[1]))
        plain = [k for k in want if k not in ("fragment_class", "owner")]
        assert set(mine) == set(want) and all(mine[k] == want[k] for k in plain), (mine, want)
        assert isinstance(mine["frag"], float) and mine["owner"].tolist() == want["owner"] and same_partition(mine["fragment_class"].tolist(), want["fragment_class"])
    keep = np.arange(len(gen[1])) % 3 != 0
    want = B.fragment_metric((gen[0][keep], gen[1][keep]), test)
    fn = S.get_fragment_metric((torch.from_numpy(test[0]), test[1]), unique=False, engine=eng)
    mine = fn((torch.from_numpy(gen[0]), gen[1]), keep=torch.from_numpy(keep))
    assert all(mine[k] == want[k] for k in plain) and mine["n_generated"] == int(keep.sum())
    from tests import scaffold_mirror as K
    gu, tu = K.unique_rows(*gen), K.unique_rows(*test)
    want = B.fragment_metric((gen[0][gu], gen[1][gu]), (test[0][tu], test[1][tu]))
    mine = S.get_fragment_metric((torch.from_numpy(test[0]), test[1]), engine=eng)((torch.from_numpy(gen[0]), gen[1]))
    assert all(mine[k] == want[k] for k in plain) and len(tu) < len(test[1])
    none = fn((torch.from_numpy(gen[0][:1]), gen[1][:1]), keep=torch.tensor([False]))
    assert math.isnan(none["frag"]) and math.isnan(none["mean_cuts"]) and none["n_generated"] == 0 and none["fragments_generated"] == 0


def test_evaluate_adds_the_entry_only_with_the_flag(monkeypatch, tmp_path, table):
    """``metrics['structure']['fragments']`` under ``config.eval.fragments`` only (the sampling and the other structure metrics are stubbed:
    this is about the wiring and the host arithmetic, on the CPU; the GPU test runs it end to end)."""
    from types import SimpleNamespace
    from diffspectra_amd import evaluate as EV
    from diffspectra_amd.config import qm9s_config
    rows, rec, n, got = table
    names = [name for name, *_ in rows]
    t_rec, t_n = torch.from_numpy(rec), torch.from_numpy(n)
    slots = [names.index(x) for x in ("methyl acetate", "ethyl acetate", "ethanol", "toluene")]
    gen_n = t_n[slots].clone()
    gen_n[3] = 0                                                                # the fourth generated record is unusable
    run = SimpleNamespace(records_by_slot=t_rec[slots].contiguous(), n_atoms=gen_n.tolist(), eng=MirrorEngine(), advance=lambda: None,
                          finish=lambda: ([], None, None), slot_ds=torch.tensor([0, 0, 1, 1]))
    cfg = qm9s_config("ir")
    cfg.eval.begin_ckpt, cfg.eval.end_ckpt, cfg.eval.ckpts, cfg.eval.top_k = 1, 1, "", 2
    (tmp_path / "checkpoints").mkdir()
    (tmp_path / "checkpoints" / "checkpoint_1.pth").write_bytes(b"")
    monkeypatch.setattr(EV, "create_model", lambda config: torch.nn.Linear(1, 1))
    monkeypatch.setattr(EV, "restore_checkpoint", lambda path, state, device: state)
    monkeypatch.setattr(EV, "get_cond_sampling_eval_fn", lambda *a, **k: SimpleNamespace(start=lambda model: run))
    monkeypatch.setattr(EV, "_structure_summary", lambda run, table, top_k: dict(success_rate=1.0))
    ds = SimpleNamespace(gt_records=t_rec, num_atom=t_n)
    plain = EV.diffspectra_evaluate(cfg, str(tmp_path), ds, structure_metrics=True)[1]["metrics"]["structure"]
    assert set(plain) == {"success_rate"}
    cfg.eval.fragments = True
    st = EV.diffspectra_evaluate(cfg, str(tmp_path), ds, structure_metrics=True)[1]["metrics"]["structure"]
    assert set(st) == {"success_rate", "fragments"}
    fr = st["fragments"]
    assert set(fr) == {"frag", "n_generated", "n_test", "fragments_generated", "fragments_test", "distinct_generated", "distinct_test", "shared",
                       "mean_cuts", "fragment_class", "owner"}
    want = B.fragment_metric((rec[slots], gen_n.numpy()), (rec, n))
    assert all(fr[k] == want[k] for k in want if k not in ("fragment_class", "owner")) and fr["owner"].tolist() == want["owner"]
    assert fr["n_generated"] == 4 and fr["fragments_generated"] == 2 + 3 + 1 and fr["mean_cuts"] == 1.0 and 0.0 < fr["frag"] < 1.0
