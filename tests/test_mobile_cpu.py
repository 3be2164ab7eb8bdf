"""CPU: the mobile-hydrogen rule of include/diffspectra_mobile.h as tests/mobile_mirror.py restates it, pinned to hand-stated molecules and
pairs (InChI cannot run where the project runs, so the table is the pin), its properties (symmetry, equivariance under renumbering, one
normal form for every single hydrogen shift, the search budget) on the table and on a seeded corpus that is asserted not to be vacuous, and
the surface of the binding that needs no device: the parsed header and the argument errors."""
import numpy as np
import pytest
import torch

from tests import graph_mirror as GM, mobile_mirror as M, structure_mirror as SM

TABLE = M.hand_table()
NAMES = [name for name, _, _ in TABLE]


def analysis(mol, max_nodes=M.DEFAULT_NODES):
    rec, n = SM.records([mol])
    return M.Analysis(rec[0], n[0], max_nodes)


@pytest.fixture(scope="module")
def corpus():
    mols = M.corpus()
    return mols, [analysis(m) for m in mols]


# ------------------------------------------------------------------------------------------------------------------ the hand table

def test_the_table_names_what_the_rule_is_pinned_on():
    assert len(TABLE) >= 24 and len(set(NAMES)) == len(NAMES)
    for name in ("4-methylimidazole", "5-methylimidazole", "3-methylpyrazole", "5-methylpyrazole", "acetamide", "acetimidic acid", "2-pyridone",
                 "2-hydroxypyridine, N=C(OH)", "2-hydroxypyridine, N-C(OH)", "4-pyridone", "acetic acid", "glycine", "glycine zwitterion", "ammonium",
                 "ammonia", "pyridine N-oxide", "acetone", "propen-2-ol", "p-aminophenol", "guanidine"):
        assert name in NAMES, name


@pytest.mark.parametrize("name", NAMES)
def test_hand_table(name):
    mol, stated = [(m, s) for nm, m, s in TABLE if nm == name][0]
    heavy = len(stated["fixed_h"])
    A = analysis(mol)
    assert A.status == M.OK and A.kept == list(range(heavy)), "every heavy atom is kept, every hydrogen folded"
    assert A.donors == stated["donors"] and A.acceptors == stated["acceptors"]
    assert A.groups == stated["groups"] and A.group_h == stated["group_h"]
    assert [A.fixed[i] for i in range(heavy)] == stated["fixed_h"] and [A.q_res[i] for i in range(heavy)] == stated["q_res"] and A.p == stated["p"]
    row = M.analyse(*[x[0] for x in SM.records([mol])])
    assert row["summary"] == (heavy, len(stated["groups"]), sum(stated["group_h"]), stated["p"]) and row["status"] == M.OK
    assert row["fixed_h"][:heavy] == stated["fixed_h"] and set(row["fixed_h"][heavy:]) == {0xff}
    assert [g for g in row["group_of"] if g != 0xff] == [g for i in range(heavy) for g, m in enumerate(stated["groups"]) if i in m]


def test_path_lengths_the_table_states():
    bonds = lambda name: sorted(len(p) - 1 for p in analysis(M.named(name)).paths)
    assert bonds("4-methylimidazole") == [2] and bonds("3-methylpyrazole") == [4] and bonds("5-methylpyrazole") == [4]
    assert bonds("2-pyridone") == [2, 6] and bonds("2-hydroxypyridine, N=C(OH)") == [2] and bonds("2-hydroxypyridine, N-C(OH)") == [6]
    assert bonds("4-pyridone") == [4, 4] and bonds("diacetamide, an iminol") == [2, 4] and bonds("glycine") == [2]


def test_an_alternating_walk_is_not_a_simple_path():
    """The odd-ring molecule of the table: the walk reaches the aldehyde oxygen, no simple path does, and the rule follows the simple path."""
    A = analysis(M.named("2-(cycloprop-2-en-1-ylidene)-2-hydroxyacetaldehyde"))
    assert A.walk_reaches(0) == {6} and A.paths == [] and A.groups == [] and A.search(0, 100) == (set(), 3)     # 0-1=2, then 2-3=4 and 2-4=3
    # where no odd ring interferes the two agree
    for name in ("2-pyridone", "3-methylpyrazole", "guanidine", "diacetamide"):
        A = analysis(M.named(name))
        assert all(A.walk_reaches(d) == {p[-1] for p in A.paths if p[0] == d} for d in A.donors), name


def test_normal_forms_of_the_table_byte_for_byte():
    rec, n = SM.records([M.named("glycine zwitterion"), M.named("ammonium"), M.named("acetate"), M.named("pyridine N-oxide")])
    out, m, source, status = M.normal_table(rec, n)
    assert status.tolist() == [0, 0, 0, 0] and m.tolist() == [5 + 1, 1 + 1, 4 + 1 + 1, 7]
    gly = out[0]
    assert gly[SM.TYPE:SM.TYPE + 6].tolist() == [2, 1, 1, 3, 3, M.GROUP_TYPE] and gly[SM.FC:SM.FC + 6].tolist() == [18, 18, 16, 16, 16, 1]
    bond = gly[SM.BOND:SM.BOND_END].reshape(29, 29)
    assert sorted(zip(*np.nonzero(np.triu(bond)))) == [(0, 1), (1, 2), (2, 3), (2, 4), (3, 5), (4, 5)] and np.array_equal(bond, bond.T) and int(bond.max()) == 1
    assert source[0].tolist() == [0, 1, 2, 3, 4] + [0xff] * 24 and not gly[SM.POS + 5 * 12:SM.TYPE].any()
    assert out[1][SM.TYPE:SM.TYPE + 2].tolist() == [2, M.PROTON_TYPE] and out[1][SM.FC:SM.FC + 2].tolist() == [16 + 3, 1]
    assert out[2][SM.TYPE + 4:SM.TYPE + 6].tolist() == [M.GROUP_TYPE, M.PROTON_TYPE] and out[2][SM.FC + 4:SM.FC + 6].tolist() == [1, 0xff]
    assert out[3][SM.FC:SM.FC + 7].tolist() == [32, 17, 17, 17, 17, 17, 0]      # N+ and O- keep their charges: 16 * (q + 1)


@pytest.mark.parametrize("a,b,verdict,layer", M.hand_pairs())
def test_hand_pairs(a, b, verdict, layer):
    assert len(M.hand_pairs()) >= 20
    got = M.identity(M.named(a), M.named(b))
    back = M.identity(M.named(b), M.named(a))
    assert got[0] == verdict and got[2] == layer and got[1] == (M.IDENTICAL if layer == 0 else M.DIFFERENT)
    assert back[:3] == got[:3], "symmetric in the pair"


# ------------------------------------------------------------------------------------------------------------------ properties

def test_equivariance_under_renumbering():
    rng = np.random.default_rng(23)
    for name, mol, _ in TABLE:
        rec, n = SM.records([mol])
        base, form = M.analyse(rec[0], n[0]), M.normal_mol(mol)[0]
        for _ in range(3):
            perm = rng.permutation(len(mol["type"]))
            new = {int(old): i for i, old in enumerate(perm)}
            moved = M.renumbered(mol, perm)
            r2, n2 = SM.records([moved])
            row = M.analyse(r2[0], n2[0])
            assert row["fixed_h"] == M.moved(base["fixed_h"], perm, 0xff) and row["q_res"] == M.moved(base["q_res"], perm, 0), name
            assert row["summary"] == base["summary"] and row["status"] == base["status"] and sorted(row["group_h"]) == sorted(base["group_h"]), name
            A, B = analysis(mol), analysis(moved)
            assert sorted(sorted(new[i] for i in g) for g in A.groups) == sorted(B.groups), name
            assert [B.group_h[B.group_of[new[g[0]]]] for g in A.groups] == A.group_h, name
            assert GM.same_graph(M.normal_mol(moved)[0], form), name


def shifts_keep_the_normal_form(mol, A):
    rec, n = SM.records([mol])
    want = M.normal_row(rec[0], n[0])
    count = 0
    for path in A.paths:
        other = M.shifted(mol, path)
        if other is None:
            continue
        r2, n2 = SM.records([other])
        got = M.normal_row(r2[0], n2[0])
        assert got[1] == want[1] and got[2] == want[2] and got[3] == want[3] and np.array_equal(got[0], want[0]), path
        count += 1
    return count


def hetero_bonded(mol):
    """An N or O bonded to an N or O: where the header's stated deviation (one pass over the input drawing) can show."""
    t, bond = np.asarray(mol["type"]), np.asarray(mol["bond"])
    het = np.isin(t, (M.N, M.O))
    return bool((bond[np.ix_(het, het)] > 0).any())


def test_every_single_shift_has_the_normal_form_of_the_original(corpus):
    """The atoms keep their numbers in ``shifted``, so the normal forms agree byte for byte: on every molecule of the table, and on every
    molecule of the corpus without a bond between two N / O atoms (with one, a shifted drawing can open a path that the input drawing does
    not have - the header's stated deviation from InChI, which iterates; the corpus holds such a case, and it is rare)."""
    total = 0
    for name, mol, _ in TABLE:
        total += shifts_keep_the_normal_form(mol, analysis(mol))
    assert total >= 20
    plain = [(m, A) for m, A in zip(*corpus) if not hetero_bonded(m)]
    assert sum(shifts_keep_the_normal_form(m, A) for m, A in plain) >= 40
    open_cases = 0
    for m, A in zip(*corpus):
        if hetero_bonded(m):
            try:
                shifts_keep_the_normal_form(m, A)
            except AssertionError:
                open_cases += 1
    assert 1 <= open_cases <= len(corpus[0]) // 50


def test_search_nodes_stay_under_the_default_budget(corpus):
    most = max(analysis(mol).nodes for _, mol, _ in TABLE)
    assert 0 < most <= 16
    assert all(A.status == M.OK for A in corpus[1]) and max(A.nodes for A in corpus[1]) <= 64 < M.DEFAULT_NODES


def test_the_search_finds_what_the_enumeration_finds(corpus):
    """Rule 6 (one double bond per interior atom, depth first, stop when every acceptor is reached) against the brute force over all simple paths."""
    for A in [analysis(mol) for _, mol, _ in TABLE] + corpus[1]:
        for d in A.donors:
            assert A.search(d, M.MAX_NODES)[0] == {p[-1] for p in A.paths if p[0] == d}


def test_the_budget_decides_reproducibly():
    mol = M.named("2-hydroxypyridine, N-C(OH)")                                  # three extensions round the ring, nothing else to try
    assert analysis(mol).nodes == 3 and analysis(mol, 3).status == M.OK and analysis(mol, 2).status == M.UNDECIDED
    assert analysis(M.named("2-pyridone")).nodes == 1                            # the path of two bonds comes first and ends the search
    rec, n = SM.records([mol])
    row = M.analyse(rec[0], n[0], 1)
    assert row["status"] == M.UNDECIDED and set(row["fixed_h"]) == {0xff} and row["summary"] == (0, 0, 0, 0) and row["nodes"] == 0
    assert M.normal_row(rec[0], n[0], 1)[1:] == (0, [0xff] * 29, M.UNDECIDED) and M.identity(mol, mol, 1)[0] == M.PAIR_UNDECIDED
    assert analysis(M.named("acetone"), 1).status == M.OK                         # no donor: nothing to search


# ------------------------------------------------------------------------------------------------------------------ the corpus

def test_the_corpus_is_not_vacuous(corpus):
    mols, found = corpus
    assert len(mols) >= 200 and all(len(m["type"]) <= 29 for m in mols)
    heavy = [int((np.asarray(m["type"]) != 0).sum()) for m in mols]
    assert max(heavy) == 9 and all(len(A.kept) == h for A, h in zip(found, heavy)), "explicit hydrogens only, every one folded"
    assert 4 * sum(bool(A.groups) for A in found) >= len(mols), "a quarter has a group"
    assert 20 * sum(any(len(p) - 1 >= 4 for p in A.paths) for A in found) >= len(mols), "one in twenty has a path of four bonds or more"
    assert sum(A.p != 0 or any(A.q_res.values()) for A in found) >= 3 and sum(len(A.groups) >= 2 for A in found) >= 2
    # closed shell: no implicit hydrogens anywhere
    for m in mols:
        val = np.asarray(m["bond"]).sum(1)
        assert all(int(v) == M.VM.VMAX[int(t), M.VM.applied_charge(int(t), int(c))] for v, t, c in zip(val, m["type"], m["fc"]))
    sizes = set()
    for m in mols:
        sizes |= ring_sizes(m)
    assert {3, 4, 5, 6} <= sizes


def ring_sizes(mol):
    """Sizes up to 6 of the shortest cycle through every ring bond."""
    bond = np.asarray(mol["bond"]) > 0
    n, out = len(bond), set()
    for i in range(n):
        for j in range(i + 1, n):
            if not bond[i, j]:
                continue
            seen, todo = {i: 0}, [i]
            while todo:
                u = todo.pop(0)
                for v in np.nonzero(bond[u])[0]:
                    if (u, int(v)) in ((i, j), (j, i)) or int(v) in seen:
                        continue
                    seen[int(v)] = seen[u] + 1
                    todo.append(int(v))
            if j in seen and seen[j] + 1 <= 6:
                out.add(seen[j] + 1)
    return out


def test_classes_of_the_table():
    mols = [m for _, m, _ in TABLE]
    cls = M.classes(mols)
    at = NAMES.index
    for a, b, verdict, _ in M.hand_pairs():
        assert (cls[at(a)] == cls[at(b)]) == (verdict == M.IDENTICAL), (a, b)
    assert len(set(cls)) < len(cls)


# ------------------------------------------------------------------------------------------------------------------ the surface

def test_header_constants_and_prototypes():
    from diffspectra_amd import abi, engine as E
    c = abi.MOBILE.consts
    assert (c["DSM_OK"], c["DSM_UNDECIDED"], c["DSM_UNUSABLE"], c["DSM_OVERFLOW"]) == (M.OK, M.UNDECIDED, M.UNUSABLE, M.OVERFLOW)
    assert (c["DSM_MAX_NODES"], c["DSM_MAX_GROUPS"], c["DSM_GROUP_TYPE"], c["DSM_PROTON_TYPE"]) == (M.MAX_NODES, M.MAX_GROUPS, M.GROUP_TYPE, M.PROTON_TYPE)
    assert (E.MOBILE_OK, E.MOBILE_UNDECIDED, E.MOBILE_UNUSABLE, E.MOBILE_OVERFLOW) == (M.OK, M.UNDECIDED, M.UNUSABLE, M.OVERFLOW)
    assert (E.MOBILE_MAX_NODES, E.MOBILE_MAX_GROUPS, E.MOBILE_GROUP_TYPE, E.MOBILE_PROTON_TYPE, E.MOBILE_DEFAULT_NODES) == \
        (M.MAX_NODES, M.MAX_GROUPS, M.GROUP_TYPE, M.PROTON_TYPE, M.DEFAULT_NODES)
    assert c["DSM_GROUP_TYPE"] > 5 == abi.BRICS.consts["DSB_ATTACH_TYPE"], "outside the alphabet of the analytics and of the BRICS fragments"
    assert abi.MOBILE.exports("dsm_") == ["dsm_mobile_records", "dsm_normal_records"]
    protos = abi.MOBILE.prototypes
    assert [t for _, t in protos["dsm_mobile_records"].params] == ["*", "*", "int64_t", "int32_t"] + ["*"] * 8
    assert [t for _, t in protos["dsm_normal_records"].params] == ["*", "*", "int64_t", "int32_t"] + ["*"] * 5
    assert [n for n, _ in protos["dsm_normal_records"].params] == ["rec", "n", "P", "max_nodes", "out_rec", "out_n", "out_source", "status", "stream"]


@pytest.mark.parametrize("call", ["mobile_records", "normal_records"])
def test_argument_errors_that_need_no_device(call):
    from diffspectra_amd import engine as E
    fn = getattr(E, call)
    rec, n = torch.zeros(3, E.RECORD_BYTES, dtype=torch.uint8), torch.zeros(3, dtype=torch.int32)
    for bad in (0, -1, E.MOBILE_MAX_NODES + 1):
        with pytest.raises(ValueError, match="max_nodes"):
            fn(rec, n, bad)
    for bad in (True, 4.0, "7"):
        with pytest.raises(TypeError, match="max_nodes"):
            fn(rec, n, bad)
    with pytest.raises(TypeError, match="rec"):
        fn(rec.to(torch.int8), n)
    with pytest.raises(ValueError, match="rec"):
        fn(rec[:, :-1], n)
    with pytest.raises(TypeError, match="n must"):
        fn(rec, n.to(torch.int64))
    with pytest.raises(ValueError, match="n must"):
        fn(rec, n[:2])
    with pytest.raises(ValueError, match="contiguous"):
        fn(torch.zeros(E.RECORD_BYTES, 3, dtype=torch.uint8).t(), n)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fn(rec, n)
