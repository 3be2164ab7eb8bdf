"""CPU: the C-ABI surface of the substructure matcher (include/diffspectra_substructure.h) and its argument checks (fake pointers: nothing that
would pass every check is ever passed), the SMARTS-subset compiler, and the mirror of tests/substructure_mirror.py on hand-stated expectations -
the pin of the definitions, since RDKit cannot run here: MACCS sets of 21 molecules, counts, anchors and covers, the functional groups of
tests/groups_mirror.py rewritten as patterns, the invariances, the node budget, and the public functions on a mirror-backed engine.  (The kernel
is checked on the GPU against the same mirror: tests/test_substructure_gpu.py.)"""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from diffspectra_amd import abi, engine as E, maccs, smarts, structure_metrics as S
from tests import graph_mirror as GM, groups_mirror as G, structure_mirror as SM, substructure_mirror as M

OK, ERR_ARG = 0, -1
FAKE = 0x1000                        # a 16-byte aligned address that is nobody's memory
FULL = 0x3FFFFFFF                    # a pattern atom without any constraint


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return E.load_library()


@pytest.fixture(scope="module")
def table():
    """The hand-stated MACCS molecules with their records and the mirror's rows over the whole MACCS table, computed once."""
    rows = M.maccs_table()
    rec, n = G.records_of([mol for _, mol, _ in rows])
    return rows, rec, n, M.analyse_table(rec, n, M.MACCS_WORDS)


@pytest.fixture(scope="module")
def derived():
    """``derived_set`` with its records, computed once."""
    mols = G.derived_set()
    rec, n = G.records_of(mols)
    return mols, rec, n


def one(mol, texts, max_nodes=M.DEFAULT_NODES):
    rec, n = G.records_of([mol])
    return M.analyse(rec[0], n[0], smarts.compile_patterns(texts), max_nodes)


# ------------------------------------------------------------------------------------------------------------------ the C-ABI surface

NAMES = ["rec", "n", "P", "patterns", "K", "max_nodes", "count", "anchors", "cover", "aromatic_mask", "aromatic_rings", "fragments", "status", "stream"]
KINDS = ["*", "*", "int64_t", "*", "int32_t", "int32_t", "*", "*", "*", "*", "*", "*", "*", "*"]


def test_header_declares_and_library_exports_the_matcher(lib):
    assert abi.SUBSTRUCTURE.exports("dsq_") == list(abi.SUBSTRUCTURE.prototypes) == ["dsq_match_records"]
    hdr = re.sub(r"/\*.*?\*/", "", open(abi.SUBSTRUCTURE.path).read(), flags=re.S)
    args = re.search(r"int\s+dsq_match_records\s*\((.*?)\)\s*;", hdr, flags=re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == NAMES
    proto = abi.SUBSTRUCTURE.prototypes["dsq_match_records"]
    assert proto.params == list(zip(NAMES, KINDS)) and proto.ret == "int"
    fn = lib.dsq_match_records
    assert fn.restype is C.c_int and list(fn.argtypes) == proto.argtypes                                      # bound from the header
    K = abi.SUBSTRUCTURE.consts
    assert (K["DSQ_OK"], K["DSQ_UNUSABLE"], K["DSQ_PATTERN_WORDS"], K["DSQ_MAX_PATTERNS"], K["DSQ_MAX_PATTERN_ATOMS"], K["DSQ_MAX_CLOSURES"]) == (0, 2, 32, 256, 14, 2)
    assert (K["DSQ_COUNT_CAP"], K["DSQ_TRUNCATED"], K["DSQ_MAX_NODES"], K["DSQ_DEFAULT_NODES"]) == (4, 128, 2 ** 24, 2 ** 18) and 1 <= K["DSQ_WAVES"] <= 16
    assert (K["DSQ_WORD_ATOM"], K["DSQ_WORD_LINK"], K["DSQ_WORD_CLOSURE"]) == (1, 15, 29)
    assert [K["DSQ_BIT_" + f] for f in ("ELEMENT", "HT", "X", "D", "RING", "CHARGE")] == [0, 10, 15, 20, 25, 27]
    assert (E.SUBSTRUCTURE_OK, E.SUBSTRUCTURE_UNUSABLE, E.SUBSTRUCTURE_TRUNCATED, E.SUBSTRUCTURE_DEFAULT_NODES) == (0, 2, 128, M.DEFAULT_NODES)
    assert (M.COUNT_CAP, M.TRUNCATED, M.MAX_ATOMS, M.MAX_CLOSURES) == (K["DSQ_COUNT_CAP"], K["DSQ_TRUNCATED"], K["DSQ_MAX_PATTERN_ATOMS"], K["DSQ_MAX_CLOSURES"])
    for other in (abi.SAMPLING, abi.TRAINING, abi.SETS, abi.VALENCE, abi.GROUPS, abi.SCAFFOLD, abi.SMILES):
        assert not other.exports("dsq_")
    text = open(abi.SUBSTRUCTURE.path).read()
    assert "UNPINNED" in text and "hydrogen-folded" in text                                                   # the deviations are stated


def test_library_without_the_symbol_is_refused(lib):
    class Hollow:
        def __getattr__(self, name):
            if name.startswith("dsq_"):
                raise AttributeError(name)
            return getattr(lib, name)
    with pytest.raises(AttributeError, match="dsq_"):
        abi.SUBSTRUCTURE.bind(Hollow())


def _call(lib, P=1, rec=FAKE, n=FAKE, patterns=FAKE, K=1, max_nodes=100, per_pattern=None, per_record=None):
    return lib.dsq_match_records(rec, n, P, patterns, K, max_nodes, *([FAKE] * 3 if per_pattern is None else per_pattern),
                                 *([FAKE] * 4 if per_record is None else per_record), None)


def test_empty_calls_launch_nothing(lib):
    assert _call(lib, P=0, rec=None, n=None, patterns=None, per_pattern=[None] * 3, per_record=[None] * 4) == OK
    assert _call(lib, P=0, rec=FAKE + 1, patterns=FAKE + 2) == OK                                           # whatever the pointers
    assert _call(lib, P=0, K=0) == OK and _call(lib, P=0, K=256, max_nodes=2 ** 24) == OK


def test_argument_errors_in_the_stated_order(lib):
    """Every pointer here is fake or NULL: a call that got past its checks would fault, so each line also shows that the check comes first."""
    # the scalars and the sizes, before "an empty call launches nothing" and before any pointer
    for P in (0, 1):
        for K in (-1, 257):
            assert _call(lib, P=P, K=K) == ERR_ARG and _call(lib, P=P, K=K, rec=None) == ERR_ARG
        for budget in (0, -5, 2 ** 24 + 1):
            assert _call(lib, P=P, max_nodes=budget) == ERR_ARG
    for P in (-1, 2 ** 31, -2 ** 40):
        assert _call(lib, P=P) == ERR_ARG and _call(lib, P=P, rec=None, n=None, per_record=[None] * 4) == ERR_ARG
    # then the table: rec, n, the alignment of rec, every per-record output
    assert _call(lib, rec=None) == ERR_ARG and _call(lib, n=None) == ERR_ARG
    for off in (1, 2, 3):
        assert _call(lib, rec=FAKE + off) == ERR_ARG
    for k in range(4):
        out = [FAKE] * 4
        out[k] = None
        assert _call(lib, per_record=out) == ERR_ARG and _call(lib, K=0, patterns=None, per_pattern=[None] * 3, per_record=out) == ERR_ARG, f"output {k}"
    # then, with K > 0, the patterns and the per-pattern outputs
    assert _call(lib, patterns=None) == ERR_ARG
    for off in (1, 2, 3):
        assert _call(lib, patterns=FAKE + off) == ERR_ARG
    for k in range(3):
        out = [FAKE] * 3
        out[k] = None
        assert _call(lib, per_pattern=out) == ERR_ARG, f"output {k}"


def test_binding_refuses_wrong_arguments():
    """Arguments are checked, never converted; and there is no CPU path."""
    rec, n = torch.zeros(4, E.RECORD_BYTES, dtype=torch.uint8), torch.full((4,), 3, dtype=torch.int32)
    words = torch.from_numpy(smarts.compile_patterns(["C", "[#8]"]))
    for call in (E.substructure_records, E.DmtEngine.substructure_records.__get__(object())):
        with pytest.raises(TypeError, match="rec"):
            call(rec.int(), n, words)
        with pytest.raises(TypeError, match="n must"):
            call(rec, n.long(), words)
        with pytest.raises(TypeError, match="patterns"):
            call(rec, n, words.long())
        with pytest.raises(ValueError, match="patterns"):
            call(rec, n, words[:, :31].contiguous())
        with pytest.raises(ValueError, match="at most 256"):
            call(rec, n, words[:1].repeat(257, 1))
        with pytest.raises(TypeError, match="max_nodes"):
            call(rec, n, words, 10.0)
        for budget in (0, 2 ** 24 + 1):
            with pytest.raises(ValueError, match="max_nodes"):
                call(rec, n, words, budget)
        with pytest.raises(RuntimeError, match="no CPU path"):
            call(rec, n, words)
    with pytest.raises(RuntimeError, match="no CPU path"):
        S.substructure_search(rec, n, ["C"])
    with pytest.raises(RuntimeError, match="no CPU path"):
        S.maccs_keys(rec, n)
    with pytest.raises(ValueError, match="int32"):
        S.substructure_search(rec, n, np.zeros((2, 31), np.int32))


# ------------------------------------------------------------------------------------------------------------------ the parser

def test_every_maccs_pattern_compiles():
    assert len(maccs.MACCS_KEYS) == 166
    texts = [t for _, alternatives, _ in maccs.MACCS_KEYS if alternatives for t in alternatives]
    assert len(texts) >= 140 and len(M.MACCS_TEXTS) <= 256
    words = smarts.compile_patterns(texts)
    assert words.dtype == np.int32 and words.shape == (len(texts), 32)
    assert all(M.well_formed([int(x) & 0xFFFFFFFF for x in w]) for w in words)
    constant = {k for k, (_, alternatives, _) in enumerate(maccs.MACCS_KEYS, start=1) if alternatives is None}
    assert constant == set(maccs.CONSTANT_ZERO) | {125, 166} and len(maccs.CONSTANT_ZERO) == 36
    assert maccs.MACCS_KEYS[139][1:] == (["[#8]"], 3) and maccs.MACCS_KEYS[117][2] == 1 and len(maccs.MACCS_KEYS[100][1]) == 7
    assert "UNPINNED" in maccs.__doc__


def test_packed_words_of_stated_examples():
    """Six patterns packed by hand from the header's layout."""
    def words(**at):
        w = np.zeros(32, np.int64)
        for k, v in at.items():
            w[int(k[1:])] = v
        return w.astype(np.int32)
    eq = lambda text, want: np.array_equal(smarts.compile_pattern(text), want)
    assert eq("*", words(w0=1, w1=FULL))
    assert eq("[#8]~[#6]", words(w0=2, w1=0x3FFFFCC0, w2=0x3FFFFC0C, w16=0xFF00))
    assert eq("[CH2]=*", words(w0=2, w1=0x3FFF9004, w2=FULL, w16=0x2200))
    aromatic_c = 0x3FFFFC08
    assert eq("c1ccccc1", words(w0=0x106, w1=aromatic_c, w2=aromatic_c, w3=aromatic_c, w4=aromatic_c, w5=aromatic_c, w6=aromatic_c,
                                w16=0x9900, w17=0x9901, w18=0x9902, w19=0x9903, w20=0x9904, w29=0x990500))
    assert eq("[!#6;!#1;!H0]", words(w0=1, w1=0x3FFFFBF0))
    assert eq("[#8]~[#7](~[#6])!@[F,Cl,Br,I]", words(w0=4, w1=0x3FFFFCC0, w2=0x3FFFFC30, w3=0x3FFFFC0C, w4=0x3FFFFD00, w16=0xFF00, w17=0xFF01, w18=0x0F01))
    # the same things written otherwise
    assert eq("[C&H2]=*", smarts.compile_pattern("[CH2]=*")) and eq("[#8]~[#6]", smarts.compile_pattern("[O,o]~[C,c]"))
    assert eq("C=1CC=1", smarts.compile_pattern("C1CC=1")) and eq("C=1CC1", smarts.compile_pattern("C1CC=1"))
    assert eq("C-,:C", smarts.compile_pattern("CC")) and eq("C!-;!=;!#;!:C", words(w0=2, w1=0x3FFFFC04, w2=0x3FFFFC04, w16=0))
    assert eq("[Cl]", words(w0=1, w1=0x3FFFFC00)) and eq("Br", words(w0=1, w1=0x3FFFFC00)) and eq("[#16]", words(w0=1, w1=0x3FFFFC00))
    assert smarts.compile_patterns([]).shape == (0, 32)


@pytest.mark.parametrize("text, names", [
    ("[$(CC)]", "recursive"), ("[C;$(C=O)]", "recursive"), ("C.C", "dots"), ("[C:1]", "atom map"), ("[C@H]", "chirality"), ("[C@@]", "chirality"),
    ("C/C=C/C", "chirality"), ("[13C]", "isotope"), ("[r5]", "'r'"), ("[x2]", "'x'"), ("[v4]", "'v'"), ("[R2]", "R2"), ("[+2]", "charges"), ("[--]", "charges"),
    ("C" * 15, "more than 14 atoms"), ("C1C2C3CC3C2C1", "more than 2 ring closures"), ("[C,H2]", "mixes properties"), ("[CH2,N]", "mixes properties"),
    ("[C,N;H2,R]", "mixes properties"), ("C=1CC-1", "two different bonds"), ("C%10CC%10", "%nn"), ("C1CC", "unfinished"), ("C(C", "unfinished"), ("C=", "unfinished"),
    ("", "needs an atom"), ("=C", "bond"), ("C11", "itself"), ("[C", "without"), ("[!*]", "!\\*"), ("[H5]", "H5"), ("C$C", "recursive"), ("C?C", "cannot read"),
])
def test_refused_constructs_raise_and_name_the_construct(text, names):
    with pytest.raises(ValueError, match=names):
        smarts.compile_pattern(text)


def test_compile_wants_text():
    with pytest.raises(TypeError):
        smarts.compile_pattern(7)
    with pytest.raises(TypeError):
        smarts.compile_patterns("CC")


# ------------------------------------------------------------------------------------------------------------------ the mirror, pinned by hand

def test_mirror_on_the_hand_stated_maccs_sets(table):
    rows, rec, n, got = table
    names = [name for name, _, _ in rows]
    assert len(rows) == 21 and len(set(names)) == 21
    assert {"biphenyl", "fluorene", "naphthalene", "methane and water", "cyclopropane", "cyclobutane", "cyclooctane", "cyclononane", "ethylene glycol",
            "glycine zwitterion"} <= set(names)
    for (name, mol, want), row in zip(rows, got):
        keys, truncated = M.maccs_of(row)
        assert row["status"] == M.OK and not truncated, name
        assert keys == want, (name, sorted(keys - want), sorted(want - keys))
        assert not keys & maccs.CONSTANT_ZERO, name


def test_both_kekule_drawings_give_equal_outputs(table):
    rows, rec, n, got = table
    by_name = {name: row for (name, _, _), row in zip(rows, got)}
    for name, mol in G.other_kekule_drawings().items():
        if name in by_name:
            r, k = G.records_of([mol])
            assert M.analyse(r[0], k[0], M.MACCS_WORDS) == by_name[name], name
    assert {"benzene", "pyridine", "naphthalene"} <= set(G.other_kekule_drawings()) & set(by_name)


def test_the_aromatic_bond_rule():
    """A bond is aromatic iff it joins consecutive atoms of an aromatic cycle: the bond between the rings of biphenyl and the five-ring bond of
    fluorene are single bonds between aromatic atoms."""
    texts = ["c-c", "c-!@c", "c-@c", "c:c", "c:!@c", "[CH2]-@c", "c=c"]
    b = one(M._biphenyl(), texts)
    assert b["count"] == [1, 1, 0, 4, 0, 0, 0] and b["cover"][0] == (1 << 0) | (1 << 6) and b["anchors"][0] == (1 << 0) | (1 << 6)
    f = one(M._fluorene(), texts)
    assert f["count"] == [1, 0, 1, 4, 0, 2, 0] and f["cover"][2] == (1 << 0) | (1 << 6) and f["cover"][5] == (1 << 5) | (1 << 11) | (1 << 12)
    assert b["aromatic_rings"] == f["aromatic_rings"] == 2 and b["aromatic_mask"] == (1 << 12) - 1 and f["aromatic_mask"] == (1 << 12) - 1


def test_counts_saturate_and_key_140(table):
    three, four, five = M.oxygen_cases()
    texts = ["[#8]", "[#8]~[#6]~[#8]", "[OH]"]
    c3, c4, c5 = (one(mol, texts) for mol in (three, four, five))
    assert c3["count"] == [3, 3, 3] and c4["count"] == [4, 4, 4] and c5["count"] == [4, 4, 4]           # pairs of O on one C: 3, 6, 6 + 1
    assert c5["anchors"][0] == 0b1111100 and c4["cover"][1] == 0b11111
    for mol, has_140, has_146 in ((three, False, True), (four, True, True), (five, True, True)):
        r, k = G.records_of([mol])
        keys = M.maccs_row(r[0], k[0])["keys"]
        assert (140 in keys, 146 in keys, 159 in keys, 164 in keys) == (has_140, has_146, True, True)


def test_anchors_and_cover_on_stated_molecules(table):
    rows, rec, n, got = table
    by_name = {name: mol for name, mol, _ in rows}
    eth = one(by_name["ethanol"], ["[#8]~[#6]", "[CH3]~*", "*~*", "[#8]~*~*", "[#1]", "*~*~*~*"])          # C0 C1 O2, hydrogens folded
    assert eth["count"] == [1, 1, 2, 1, 0, 0] and eth["anchors"] == [0b100, 0b001, 0b111, 0b100, 0, 0] and eth["cover"] == [0b110, 0b011, 0b111, 0b111, 0, 0]
    assert (eth["aromatic_mask"], eth["aromatic_rings"], eth["fragments"], eth["status"]) == (0, 0, 1, M.OK)
    pyr = one(by_name["pyridine"], ["n", "c:n", "n1ccccc1", "[#7;R]~*"])                                   # N0, C1..C5
    assert pyr["count"] == [1, 2, 1, 2] and pyr["anchors"] == [1, 0b100010, 1, 1] and pyr["cover"] == [1, 0b100011, 0b111111, 0b100011]
    assert (pyr["aromatic_mask"], pyr["aromatic_rings"]) == (0b111111, 1)
    h2 = one(G.VM.molecule([0, 0], [(0, 1, 1)]), ["[#1]", "[#1]~[#1]", "*"])                                # H2 stays matchable
    assert h2["count"] == [2, 1, 2] and h2["fragments"] == 1
    both = one(by_name["methane and water"], ["*", "[#6]", "*~*"])
    assert both["count"] == [2, 1, 0] and both["fragments"] == 2 and both["anchors"][0] == 0b11


GROUP_PATTERNS = {0: "[C;X4]", 1: "[C;X3]=[C;X3]", 2: "[C;X2]#C", 3: "c", 4: "[O;X2;H1]-[#6]", 5: "[#6]-[O;X2;H0]-[#6]", 10: "F-[#6]", 14: "[N;X1]#[C;X2]"}


def test_functional_groups_as_patterns_agree_with_the_groups_mirror(derived):
    """Eight groups of diffspectra_groups.h rewritten as patterns give, on the whole derived set, the bits of ``groups_mirror.analyse``."""
    mols, rec, n = derived
    words = smarts.compile_patterns(list(GROUP_PATTERNS.values()))
    seen = {g: 0 for g in GROUP_PATTERNS}
    for r, k in zip(rec, n):
        mine, theirs = M.analyse(r, k, words), G.analyse(r, k)
        assert mine["aromatic_mask"] == theirs["aromatic_mask"] and mine["status"] == M.OK
        for column, g in enumerate(GROUP_PATTERNS):
            assert (mine["count"][column] > 0) == bool((theirs["groups"] >> g) & 1), (G.NAMES[g], mine["count"][column])
            seen[g] += mine["count"][column] > 0
    assert all(5 <= v <= len(mols) - 5 for v in seen.values()), seen


# ------------------------------------------------------------------------------------------------------------------ invariances

def test_mirror_is_invariant_under_renumbering(table):
    rows, rec, n, got = table
    rng = np.random.default_rng(23)
    remap = lambda mask, perm: sum(1 << i for i in range(len(perm)) if (mask >> int(perm[i])) & 1)
    for (name, mol, _), row in zip(rows, got):
        perm = rng.permutation(len(mol["type"]))
        new = dict(pos=mol["pos"][perm], type=mol["type"][perm].copy(), fc=mol["fc"][perm].copy(), bond=mol["bond"][np.ix_(perm, perm)].copy())
        r, k = G.records_of([new])
        h = M.analyse(r[0], k[0], M.MACCS_WORDS)
        assert h["count"] == row["count"] and (h["aromatic_rings"], h["fragments"], h["status"]) == (row["aromatic_rings"], row["fragments"], M.OK), name
        assert h["aromatic_mask"] == remap(row["aromatic_mask"], perm), name
        assert h["anchors"] == [remap(m, perm) for m in row["anchors"]] and h["cover"] == [remap(m, perm) for m in row["cover"]], name


def test_explicit_and_implicit_hydrogens_give_equal_outputs(table):
    """The heavy atoms come first in every molecule, so the masks are equal too."""
    rows, rec, n, got = table
    by_name = {name: row for (name, _, _), row in zip(rows, got)}
    cases = G.implicit_hydrogen_cases()
    assert {name for name, _ in cases} >= {"ethanol", "methane", "benzene", "acetic acid"}
    for name, mol in cases:
        r, k = G.records_of([mol])
        assert M.analyse(r[0], k[0], M.MACCS_WORDS) == by_name[name], name


def test_garbage_is_ignored_and_unusable_records_give_zeros(table):
    rows, rec, n, got = table
    K = len(M.MACCS_WORDS)
    zero = dict(count=[0] * K, anchors=[0] * K, cover=[0] * K, aromatic_mask=0, aromatic_rings=0, fragments=0, status=M.UNUSABLE)
    at = [name for name, _, _ in rows].index("fluorene")
    base, k = rec[at], int(n[at])
    assert M.analyse(base, 0, M.MACCS_WORDS) == zero and M.analyse(base, -2, M.MACCS_WORDS) == zero
    bad = base.copy()
    bad[SM.TYPE + 3] = 5
    assert M.analyse(bad, k, M.MACCS_WORDS) == zero
    bad = base.copy()
    bad[SM.BOND + 2 * 29 + 9] = 4
    assert M.analyse(bad, k, M.MACCS_WORDS) == zero
    fine = base.copy()                                                          # the lower triangle, the diagonal, atoms >= n and the pad are not looked at
    fine[SM.BOND + 9 * 29 + 2] = fine[SM.BOND + 4 * 29 + 4] = fine[SM.TYPE + k] = fine[SM.FC + k + 1] = fine[SM.BOND + 1 * 29 + k] = 200
    fine[SM.BOND_END:] = 0xEE
    assert M.analyse(fine, k, M.MACCS_WORDS) == got[at]


def test_malformed_patterns_match_nothing(table):
    rows, rec, n, got = table
    good = smarts.compile_pattern("*1~*~*~*~*~*~1").astype(np.int64)
    cases = []
    for word, value in ((0, 0), (0, 15), (0, 6 | (3 << 8)), (0, 255 | (255 << 8)), (17, 2 | 0xFF00), (17, 200 | 0xFF00), (29, 5 | (5 << 8) | (0xFF << 16)),
                        (29, 3 | (2 << 8) | (0xFF << 16)), (29, 0 | (6 << 8) | (0xFF << 16)), (29, 0 | (77 << 8) | (0xFF << 16))):
        w = good.copy()
        w[word] = value
        cases.append(w)
    cases.append(np.full(32, -1, np.int64))
    words = np.stack(cases).astype(np.int32)
    at = [name for name, _, _ in rows].index("benzene")
    out = M.analyse(rec[at], n[at], words)
    assert out["count"] == [0] * len(cases) and out["anchors"] == [0] * len(cases) and out["cover"] == [0] * len(cases) and out["aromatic_mask"] == 0b111111
    assert M.analyse(rec[at], n[at], good[None].astype(np.int32))["count"] == [1]


# ------------------------------------------------------------------------------------------------------------------ the node budget

def test_default_budget_truncates_nothing_on_the_test_molecules(table, derived):
    """A condition, not a measurement: under the full MACCS table with DSQ_DEFAULT_NODES no entry of the hand tables or of the derived set is
    truncated."""
    rows, rec, n, got = table
    assert not any(c & M.TRUNCATED for row in got for c in row["count"])
    extra = [mol for _, mol, _, _ in G.hand_table()] + [G.quaterphenyl_29()]
    r2, n2 = G.records_of(extra)
    mols, r3, n3 = derived
    for r, k in list(zip(r2, n2)) + list(zip(r3, n3)):
        row = M.analyse(r, k, M.MACCS_WORDS)
        assert row["status"] == M.OK and not any(c & M.TRUNCATED for c in row["count"])


def test_k29_is_truncated_with_the_defined_partial_outputs():
    """The complete graph on 29 carbons against the 14-atom cycle: every atom is a ring atom and every bond a ring bond, so a search walks 0, 1,
    2, ... in index order.  12 assignments complete nothing; the 13th completes the first embedding - atoms 0..13 for a start below 14, the start
    and 0..12 otherwise; with 500 every start completes many."""
    (rec,), (n,) = [x[:1] for x in SM.records([GM.k29()])]
    words = smarts.compile_patterns([maccs._cycle(14), "[#7]", maccs._cycle(8)])
    everyone = (1 << 29) - 1
    out = M.analyse(rec, n, words, 12)
    assert out["count"] == [M.TRUNCATED, 0, 4 | M.TRUNCATED] and out["anchors"][0] == 0 and out["cover"][0] == 0
    out = M.analyse(rec, n, words, 13)
    assert out["count"] == [4 | M.TRUNCATED, 0, 4 | M.TRUNCATED] and out["anchors"][0] == everyone and out["cover"][0] == everyone
    out = M.analyse(rec, n, words, 500)
    assert out["count"] == [4 | M.TRUNCATED, 0, 4 | M.TRUNCATED] and out["anchors"] == [everyone, 0, everyone] and out["cover"] == [everyone, 0, everyone]
    assert (out["aromatic_mask"], out["aromatic_rings"], out["fragments"], out["status"]) == (0, 0, 1, M.OK)
    one_start = M.match(M.Graph(rec, n), words[0], 13)
    assert one_start["count"] == 4 | M.TRUNCATED


# ------------------------------------------------------------------------------------------------------------------ the public interface

class MirrorEngine:
    """An engine that answers the matcher call from the mirror: what ``structure_metrics`` does around the kernel, without it."""

    def substructure_records(self, rec, n, patterns, max_nodes=M.DEFAULT_NODES):
        K = patterns.shape[0]
        rows = M.analyse_table(rec.numpy(), n.numpy(), patterns.numpy(), max_nodes)
        return tuple(torch.from_numpy(a) for a in M.as_arrays(rows, K))


def test_public_interface_on_the_mirror_engine(table):
    rows, rec, n, got = table
    names = [name for name, _, _ in rows]
    eng = MirrorEngine()
    t_rec, t_n = torch.from_numpy(rec), torch.from_numpy(n)
    found = S.substructure_search(t_rec, t_n.tolist(), ["c", "[OH]", "*1~*~*~1"], engine=eng)
    assert isinstance(found, S.SubstructureMatches) and found.count.dtype == torch.uint8 and found.count.shape == (len(rows), 3) and not found.truncated.any()
    assert found.has(0).tolist() == [162 in want for _, _, want in rows] and found.has(2).tolist() == [22 in want for _, _, want in rows]
    assert found.has(1).tolist() == [139 in want and "water" not in name for name, _, want in rows]        # water's O has two hydrogens
    compiled = S.substructure_search(t_rec, t_n, smarts.compile_patterns(["c", "[OH]", "*1~*~*~1"]), engine=eng)
    assert all(torch.equal(a, b) for a, b in zip(found, compiled))
    k29 = [torch.from_numpy(np.asarray(x[:1])) for x in SM.records([GM.k29()])]
    cut = S.substructure_search(k29[0], k29[1].to(torch.int32), [maccs._cycle(14)], max_nodes=500, engine=eng)
    assert cut.count.tolist() == [[4]] and cut.truncated.tolist() == [[True]]
    none = S.substructure_search(t_rec, t_n, [], engine=eng)
    assert none.count.shape == (len(rows), 0) and none.fragments.tolist() == [2 if name == "methane and water" else 1 for name in names]
    # the MACCS keys
    keys = S.maccs_keys(t_rec, t_n, engine=eng)
    assert isinstance(keys, S.MaccsKeys) and keys.bits.shape == (len(rows), 167) and keys.bits.dtype == torch.bool and not keys.truncated.any()
    for p, (name, _, want) in enumerate(rows):
        assert set(torch.nonzero(keys.bits[p]).reshape(-1).tolist()) == want, name
    # pairs: ethanol against (ethanol, ethylene glycol, a row outside, methane), benzene against (pyridine, n = 0, benzene, a row outside)
    pick = lambda *ns: [names.index(x) for x in ns]
    prb_rows = pick("ethanol", "ethylene glycol", "water", "methane", "pyridine", "benzene", "benzene", "water")
    prb_n = t_n[prb_rows].clone()
    prb_n[5] = 0
    ref_index = torch.tensor(pick("ethanol", "ethanol") + [-1] + pick("ethanol", "benzene", "benzene", "benzene") + [len(rows)])
    out = S.maccs_similarity_batch(t_rec[prb_rows].contiguous(), prb_n, t_rec, t_n, ref_index=ref_index, engine=eng)
    assert isinstance(out, S.MaccsSimilarity) and out.tanimoto.dtype == torch.float64
    assert out.status.tolist() == [0, 0, 3, 0, 0, 2, 0, 3] and out.valid.tolist() == [True, True, False, True, True, False, True, False]
    assert out.common.tolist() == [9, 7, -1, 1, 3, -1, 3, -1] and out.either.tolist() == [9, 18, -1, 9, 8, -1, 3, -1]
    sim = out.tanimoto.tolist()
    assert sim[0] == 1.0 and sim[1] == 7 / 18 and sim[2] != sim[2] and sim[3] == 1 / 9 and sim[4] == 3 / 8 and sim[5] != sim[5] and sim[6] == 1.0 and sim[7] != sim[7]
    top = S.topk_maccs(out.tanimoto, out.status, 4)
    assert top["best"].tolist() == [1.0, 1.0] and top["best_index"].tolist() == [0, 2] and float(top["mean_best"]) == 1.0
    assert not out.truncated.any()
    cut = S.maccs_similarity_batch(k29[0], k29[1].to(torch.int32), k29[0], k29[1].to(torch.int32), max_nodes=40, engine=eng)
    assert cut.truncated.tolist() == [True] and cut.status.tolist() == [0] and cut.tanimoto.tolist() == [1.0]
    with pytest.raises(ValueError, match="top_k"):
        S.topk_maccs(out.tanimoto, out.status, 3)
    with pytest.raises(ValueError, match="ground-truth row"):
        S.maccs_similarity_batch(t_rec, t_n, t_rec[:2].contiguous(), t_n[:2], engine=eng)
    # neither molecule sets a key: 1.0
    h2 = G.records_of([G.VM.molecule([0, 0], [(0, 1, 1)])])
    lone = S.maccs_similarity_batch(torch.from_numpy(h2[0]), torch.from_numpy(h2[1]), torch.from_numpy(h2[0]), torch.from_numpy(h2[1]), engine=eng)
    assert lone.either.tolist() == [0] and lone.tanimoto.tolist() == [1.0]


def test_evaluate_adds_the_entry_only_with_the_flag(monkeypatch, tmp_path, table):
    """``metrics['structure']['maccs']`` under ``config.eval.maccs`` only (the sampling and the other structure metrics are stubbed: this is about
    the wiring and the host arithmetic, on the CPU; the GPU test runs it end to end)."""
    from types import SimpleNamespace
    from diffspectra_amd import evaluate as EV
    from diffspectra_amd.config import qm9s_config
    rows, rec, n, got = table
    names = [name for name, _, _ in rows]
    t_rec, t_n = torch.from_numpy(rec), torch.from_numpy(n)
    slots = [names.index(x) for x in ("ethanol", "ethylene glycol", "pyridine", "benzene")]
    gen_n = t_n[slots].clone()
    gen_n[3] = 0                                                                # the fourth generated record is unusable
    run = SimpleNamespace(records_by_slot=t_rec[slots].contiguous(), n_atoms=gen_n.tolist(), eng=MirrorEngine(), advance=lambda: None,
                          finish=lambda: ([], None, None), slot_ds=torch.tensor([names.index("ethanol")] * 2 + [names.index("benzene")] * 2))
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
    cfg.eval.maccs = True
    st = EV.diffspectra_evaluate(cfg, str(tmp_path), ds, structure_metrics=True)[1]["metrics"]["structure"]
    assert set(st) == {"success_rate", "maccs"}
    mk = st["maccs"]
    assert set(mk) == {"tanimoto", "status", "mean", "scored", "truncated", "top_k"} and mk["truncated"] == 0
    assert mk["status"].tolist() == [0, 0, 0, 2] and mk["scored"] == 3 and mk["mean"] == (1.0 + 7 / 18 + 3 / 8) / 3
    assert mk["top_k"]["best"].tolist() == [1.0, 3 / 8] and mk["top_k"]["best_index"].tolist() == [0, 0]
    cfg.eval.top_k = 1
    assert "top_k" not in EV.diffspectra_evaluate(cfg, str(tmp_path), ds, structure_metrics=True)[1]["metrics"]["structure"]["maccs"]
