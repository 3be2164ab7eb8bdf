"""CPU: the key-level identity of include/diffspectra_key.h as tests/key_mirror.py restates it - the normal form of diffspectra_mobile.h and
the stereo verdicts of diffspectra_stereo.h at once.  InChI cannot run where the project runs, so the hand-stated table is the pin; every
number built on these verdicts restates InChI as remembered and is UNPINNED against it.  Then the properties: symmetry, invariance under
renumbering and rigid motion, reflection, the twin rule, and three laws that tie this level to the two it combines - on seeded sets that
are asserted not to be vacuous - and the surface of the binding that needs no device: the parsed header and the argument errors."""
import collections
import math

import numpy as np
import pytest

from tests import key_mirror as K, mobile_mirror as MM, stereo_mirror as ST, structure_mirror as SM

MOLS = K.hand_molecules()
PAIRS = K.hand_pairs()
OK_ARG, ERR_ARG = 0, -1
FAKE = 0x1000                        # an aligned address that is nobody's memory: an argument error returns before anything is read


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from diffspectra_amd import engine as E
    g.build()
    return E.load_library()


@pytest.fixture(scope="module")
def law2():
    prb, ref, names = K.law2_pairs()
    return [(a, b, name, K.compare(a, b), ST.compare(a, b)) for a, b, name in zip(prb, ref, names)]


# ------------------------------------------------------------------------------------------------------------------ a. the header

def test_header_constants_and_prototypes(lib):
    from diffspectra_amd import abi, engine as E
    c = abi.KEY.consts
    assert (c["DSI_KIND_MASK"], c["DSI_KIND_NONE"], c["DSI_KIND_CENTRE"], c["DSI_KIND_END"]) == (3, 0, K.KIND_CENTRE, K.KIND_END)
    assert (c["DSI_FLAG_ASSIGNED"], c["DSI_FLAG_SIGN"], c["DSI_FLAG_HSLOT"], c["DSI_NO_PARTNER"]) == (K.ASSIGNED, K.SIGN, K.HSLOT, K.NO_PARTNER)
    assert c["DSI_SITE_BYTES"] == 2 * K.W and c["DSI_NUM_MASKS"] == len(K.MASKS) == abi.STEREO.consts["DSC_NUM_MASKS"] + 2
    assert (c["DSI_MASK_MOBILE_BOND"], c["DSI_MASK_RING_BOND"]) == (K.MASKS.index("mobile_bond"), K.MASKS.index("ring_bond"))
    assert (E.KEY_KIND_MASK, E.KEY_KIND_CENTRE, E.KEY_KIND_END, E.KEY_FLAG_ASSIGNED, E.KEY_FLAG_SIGN, E.KEY_FLAG_HSLOT, E.KEY_NO_PARTNER, E.KEY_NUM_MASKS) == \
        (3, K.KIND_CENTRE, K.KIND_END, K.ASSIGNED, K.SIGN, K.HSLOT, K.NO_PARTNER, 9)
    s = abi.STEREO.consts
    assert [s["DSC_" + k] for k in ("DIFFERENT", "IDENTICAL", "UNDECIDED", "INVALID", "MIRROR", "STEREOISOMER", "UNASSIGNED")] == \
        [K.DIFFERENT, K.IDENTICAL, K.UNDECIDED, K.INVALID, K.MIRROR, K.STEREOISOMER, K.UNASSIGNED]
    assert abi.KEY.exports("dsi_") == ["dsi_key_sites", "dsi_key_identity_records"] and sorted(abi.KEY.prototypes) == sorted(abi.KEY.exports("dsi_"))
    for name in abi.KEY.prototypes:
        assert hasattr(lib, name), name                                              # every declared symbol is exported
    protos = abi.KEY.prototypes
    assert [t for _, t in protos["dsi_key_sites"].params] == ["*", "*", "int64_t", "int32_t", "double", "double"] + ["*"] * 6
    assert [n for n, _ in protos["dsi_key_identity_records"].params] == [
        "prb_rec", "prb_n", "P", "ref_rec", "ref_n", "M", "ref_index", "prb_site", "ref_site", "max_nodes", "exhaustive", "verdict", "nodes", "found",
        "sites", "map", "stream"]


def test_argument_errors_in_contract_order(lib):
    from diffspectra_amd import abi
    nodes_most, graph_most = abi.MOBILE.consts["DSM_MAX_NODES"], abi.SAMPLING.consts["DS_GRAPH_MAX_NODES"]
    sites = lambda rec=FAKE, n=FAKE, P=1, nodes=64, mv=0.5, mp=0.5, outs=(FAKE,) * 5: lib.dsi_key_sites(rec, n, P, nodes, mv, mp, *outs, None)
    assert sites(P=0, rec=None, n=None, outs=(None,) * 5) == OK_ARG                   # P = 0 launches nothing whatever the pointers
    for bad in (dict(nodes=0), dict(nodes=nodes_most + 1), dict(mv=-1.0), dict(mv=float("nan")), dict(mp=-0.5), dict(mp=float("nan")), dict(P=-1),
                dict(P=2 ** 31), dict(rec=None), dict(n=None), dict(rec=FAKE + 2)):
        assert sites(**bad) == ERR_ARG, bad
        assert sites(**{**bad, "P": bad.get("P", 0)}) == (ERR_ARG if set(bad) & {"nodes", "mv", "mp", "P"} else OK_ARG), bad   # the scalars and the sizes come first
    for k in range(5):
        assert sites(outs=tuple(None if j == k else FAKE for j in range(5))) == ERR_ARG

    def pairs(P=1, M=1, prb=FAKE, prb_n=FAKE, ref=FAKE, ref_n=FAKE, index=None, prb_site=FAKE, ref_site=FAKE, nodes=64, exhaustive=0, outs=(FAKE,) * 5):
        return lib.dsi_key_identity_records(prb, prb_n, P, ref, ref_n, M, index, prb_site, ref_site, nodes, exhaustive, *outs, None)
    assert pairs(P=0, M=0, prb=None, prb_n=None, ref=None, ref_n=None, prb_site=None, ref_site=None, outs=(None,) * 5) == OK_ARG
    for bad in (dict(nodes=-1), dict(nodes=graph_most + 1), dict(exhaustive=2), dict(exhaustive=-1), dict(M=-1), dict(P=-1), dict(P=2 ** 31)):
        assert pairs(**bad) == ERR_ARG, bad
        assert pairs(**{**bad, "P": bad.get("P", 0)}) == ERR_ARG, bad                  # before P = 0 is looked at
    for bad in (dict(prb=None), dict(prb_n=None), dict(prb=FAKE + 1), dict(ref=None), dict(ref_n=None), dict(ref=FAKE + 2), dict(M=0, index=None),
                dict(prb_site=None), dict(ref_site=None)):
        assert pairs(**bad) == ERR_ARG, bad
        assert pairs(**{**bad, "P": 0}) == OK_ARG, bad                                 # the pointers are looked at for P > 0 only
    for k in range(5):
        assert pairs(outs=tuple(None if j == k else FAKE for j in range(5))) == ERR_ARG


# ------------------------------------------------------------------------------------------------------------------ b. the hand table

def test_the_table_names_what_the_definition_is_pinned_on():
    for name in ("lactic acid", "alanine zwitterion", "4-(1-fluoroethyl)imidazole", "5-(1-fluoroethyl)imidazole", "(E)-crotonic acid", "(Z)-crotonic acid",
                 "(E)-N-methylacetimidic acid", "N-methylacetamide", "(E)-3-hydroxyacrolein", "(E)-acetaldoxime", "2-pyridone", "2-hydroxypyridine, N-C(OH)",
                 "o-xylene, C1=C2", "(Z)-1,2-difluoroethene", "fumaric acid", "maleic acid", "flattened 1-fluoroethanol", "1,3-difluoroallene"):
        assert name in MOLS, name
    assert len(PAIRS) >= 25 and len(K.stereo_table_pairs()) >= 20
    assert {v for _, _, v, _ in PAIRS} == {K.DIFFERENT, K.IDENTICAL, K.MIRROR, K.STEREOISOMER, K.UNASSIGNED}
    assert {layer for _, _, _, layer in PAIRS} >= {0, 1, -1}


@pytest.mark.parametrize("pair", PAIRS, ids=[f"{a} / {b}" for a, b, _, _ in PAIRS])
def test_hand_pairs(pair):
    a, b, verdict, layer = pair
    got_verdict, strict, got_layer = K.identity(MOLS[a], MOLS[b])
    assert got_verdict == verdict, (got_verdict, strict)
    if layer is not None:
        assert got_layer == layer, (got_layer, strict)
    r = K.compare(MOLS[a], MOLS[b])
    for kind, code in (("same", K.IDENTICAL), ("mirror", K.MIRROR), ("iso", K.STEREOISOMER)):
        for image in r["maps"][kind][:1]:
            if verdict == code:
                assert K.map_claim(MOLS[a], MOLS[b], image + [-1] * (K.W - len(image)), verdict)


@pytest.mark.parametrize("name", sorted(K.hand_sites()))
def test_hand_sites(name):
    """Centres, hydrogen slots, E/Z sites and the rejected bonds as stated by hand, in original atoms."""
    stated, P = K.hand_sites()[name], K.Perception(MOLS[name])
    assert P.status == K.OK
    src = P.source
    on_site = {s["atom"] for s in P.tetra} | {x for s in P.ez for x in (s["a"], s["b"])}
    assert {src[s["atom"]] for s in P.tetra} == stated["centres"]
    assert {src[x] for x in P.hatom if x in on_site} == stated["hslots"]
    assert {frozenset((src[s["a"]], src[s["b"]])) for s in P.ez} == stated["ez"]
    assert {src[x] for x in P.mobile} == stated["mobile"] and {src[x] for x in P.ring} == stated["ring"]
    assert all(s["assigned"] for s in P.tetra + P.ez)
    row = K.site_rows(MOLS[name], found=P)
    assert row["status"] == K.OK and row["nodes"] == P.nodes
    assert bin(row["masks"][0]).count("1") == len(stated["centres"]) and bin(row["masks"][3]).count("1") == 2 * len(stated["ez"])


def test_the_consequences_the_header_states():
    sites = lambda name: K.compare(MOLS[name], MOLS[name])["sites"][:2]
    assert sites("(E)-N-methylacetimidic acid") == [0, 0] and sites("N-methylacetamide") == [0, 0]           # no site in either form
    assert sites("(E)-3-hydroxyacrolein") == [0, 0]
    assert sites("(E)-acetaldoxime") == [0, 1]                                                               # the oxime keeps its site
    assert sites("(E)-crotonic acid") == sites("(E)-crotonic acid, the other oxygen") == [0, 1]              # whichever oxygen carries the hydrogen
    assert sites("2-pyridone") == [0, 0] and sites("o-xylene, C1=C2") == [0, 0]                              # ring double bonds are never sites
    # the same molecules at the level of diffspectra_stereo.h, as drawn: sites that this level drops
    assert ST.compare(MOLS["(E)-N-methylacetimidic acid"], MOLS["(Z)-N-methylacetimidic acid"])["verdict"] == K.STEREOISOMER
    assert ST.compare(MOLS["(E)-3-hydroxyacrolein"], MOLS["(Z)-3-hydroxyacrolein"])["verdict"] == K.STEREOISOMER


@pytest.mark.parametrize("row", K.stereo_table_pairs(), ids=[name for name, _, _, _ in K.stereo_table_pairs()])
def test_the_stereo_table_at_this_level(row):
    """Every pair of stereo_mirror.hand_table() whose drawings have no mobile group and no ring double bond: the verdict stated there.  One
    exception, stated by hand: '1-fluoroethanol / C=O' edits a bond order and over-fills the oxygen's valence (O(H)=C), so no hydrogen
    count changes; the normal form does not compare bond orders and the pair is IDENTICAL here (law 1 below: the mobile verdict is 1).  A
    changed skeleton that is DIFFERENT at this level is in the hand pairs."""
    name, a, b, verdict = row
    assert K.plain(a) and K.plain(b)
    want = K.IDENTICAL if name == "1-fluoroethanol / C=O" else verdict
    assert K.compare(a, b)["verdict"] == want
    assert (MM.identity(a, b)[0] == MM.IDENTICAL) == (want != K.DIFFERENT)


def test_a_changed_skeleton_is_different():
    assert K.identity(MOLS["2-fluoroethanol"], MOLS["1-fluoroethanol"]) == (K.DIFFERENT, K.DIFFERENT, -1)
    assert K.compare(MOLS["1-fluoroethanol"], ST.difluoroethene(True))["verdict"] == K.DIFFERENT


# ------------------------------------------------------------------------------------------------------------------ c. invariances

def invariance_set():
    """(generated, ground truth) pairs the invariances run on: the hand pairs and every tenth pair of the law-2 set."""
    prb, ref, _ = K.law2_pairs()
    return [(MOLS[a], MOLS[b]) for a, b, _, _ in PAIRS] + list(zip(prb, ref))[::10]


def test_symmetric_up_to_the_roles_in_sites():
    for a, b in invariance_set():
        ab, ba = K.compare(a, b), K.compare(b, a)
        assert ab["verdict"] == ba["verdict"] and ab["found"] == ba["found"]
        assert ab["sites"][2:] == ba["sites"][:1:-1]
        if ab["verdict"] != K.DIFFERENT:
            assert ab["sites"][:2] == ba["sites"][:2], "an isomorphism maps sites onto sites only where the counts agree - and they do here"


def test_unchanged_by_renumbering_and_rigid_motion():
    rng = np.random.default_rng(20261102)
    for a, b in invariance_set():
        want = K.compare(a, b)
        for a2, b2 in ((ST.renumbered(a, rng), b), (a, ST.renumbered(b, rng)), (ST.renumbered(a, rng), ST.renumbered(b, rng))):
            got = K.compare(a2, b2)
            assert (got["verdict"], got["found"], got["sites"]) == (want["verdict"], want["found"], want["sites"])


def test_reflection_exchanges_identical_and_mirror_where_the_molecule_is_chiral():
    seen = collections.Counter()
    for a, b in invariance_set():
        want, got = K.compare(a, b), K.compare(K.reflected(a), b)
        if want["verdict"] in (K.IDENTICAL, K.MIRROR):
            chiral = want["found"][1] == 0 or want["found"][2] == 0            # no phi of the other kind: the molecule has no mirror automorphism
            if chiral and want["sites"][0] > 0:
                assert got["verdict"] == (K.MIRROR if want["verdict"] == K.IDENTICAL else K.IDENTICAL)
                assert got["found"] == [want["found"][0], want["found"][2], want["found"][1]]
                seen["exchanged"] += 1
            else:
                assert got["verdict"] == K.IDENTICAL == want["verdict"]
                seen["achiral"] += 1
        else:
            assert got["verdict"] == want["verdict"]
            seen["other"] += 1
    assert seen["exchanged"] >= 5 and seen["achiral"] >= 10 and seen["other"] >= 5, seen


def test_the_twin_rule_by_brute_force():
    """Isomorphisms with ordinals times the product of the factorials of the twin classes = isomorphisms without ordinals, on the small entries."""
    checked = 0
    isopropanol = K.Builder()                                # (CH3)2CH-OH: the two methyl groups are twins on the normal form, so the carbon is no centre
    c = isopropanol.atom(K.C, (0, 0, 0))
    isopropanol.methyl(K.T[0] * 1.5, c, 1, 0)
    isopropanol.methyl(K.T[1] * 1.5, c, 1, 1)
    o = isopropanol.atom(K.O, K.T[2] * 1.4, c)
    isopropanol.atom(K.H, K.T[2] * 2.3, o)
    isopropanol.atom(K.H, K.T[3] * 1.1, c)
    small = {name: MOLS[name] for name in ("lactic acid", "alanine zwitterion", "(E)-crotonic acid", "fumaric acid", "N-methylacetamide", "o-xylene, C1=C2",
                                           "1,3-difluoroallene", "(Z)-1,2-difluoroethene")}
    small.update({"isopropanol": isopropanol.done(), "neopentane": ST.neopentane(), "cis-1,3-difluorocyclobutane": ST.difluorocyclobutane(True), "2,3-difluorobutane": ST.difluorobutane(True)})
    for name, mol in small.items():
        P = K.Perception(mol)
        with_ordinals = sum(1 for _ in ST.isomorphisms(P.nf, P.nf, P.ordinal, P.ordinal))
        zero = [0] * P.total
        without = sum(1 for _ in ST.isomorphisms(P.nf, P.nf, zero, zero))
        are_twins, _, _ = ST.twins_of(P.nf)
        classes = collections.Counter(min(j for j in range(P.total) if j == i or are_twins(i, j)) for i in range(P.total))
        assert without == with_ordinals * math.prod(math.factorial(c) for c in classes.values()), name
        checked += any(c > 1 for c in classes.values())
    P = K.Perception(small["isopropanol"])
    assert P.tetra == [] and sum(P.twin) == 2 and sorted(P.ordinal) == [0, 0, 0, 1]
    assert checked >= 2


# ------------------------------------------------------------------------------------------------------------------ d. law 1

def test_law_1_the_main_layer_is_the_mobile_verdict(law2):
    """The key verdict is in {1, 4, 5, 6} exactly when the mobile verdict of the pair is 1, and 0 exactly when that is 0."""
    names = sorted(MOLS)
    pairs = [(MOLS[a], MOLS[b]) for a, b, _, _ in PAIRS] + [(a, b) for a, b, _, _, _ in law2] + [(s, m) for _, _, m, s in K.shifted_forms()]
    pairs += [(MOLS[a], MOLS[b]) for a, b in zip(names, names[1:])]                   # neighbours in the alphabet: mostly other molecules
    seen = collections.Counter()
    for a, b in pairs:
        mobile, key = MM.identity(a, b)[0], K.compare(a, b)["verdict"]
        assert (key in (K.IDENTICAL, K.MIRROR, K.STEREOISOMER, K.UNASSIGNED)) == (mobile == MM.IDENTICAL)
        assert (key == K.DIFFERENT) == (mobile == MM.DIFFERENT)
        seen[mobile] += 1
    assert seen[MM.IDENTICAL] >= 100 and seen[MM.DIFFERENT] >= 20


# ------------------------------------------------------------------------------------------------------------------ e. law 2

LAW2_PAIRS, LAW2_FOLD_TWINS = 217, 14      # counted on the CPU with the mirrors alone


def test_law_2_plain_molecules_get_the_stereo_verdict(law2):
    """On pairs where neither side has a mobile group, a proton transfer or a ring double bond (``key_mirror.plain``) and both records are
    within their valences, the key verdict equals stereo_mirror.compare's.  One kind of pair is counted, listed and excluded: a side with
    twins that only the fold makes (two NH2 or OH groups on one atom: leaves of the normal form, not of the drawing).  The header takes
    twins on the normal form, so the atom that carries them is no centre here, while diffspectra_stereo.h calls it a site and finds its
    symmetry as an automorphism - the verdicts then differ exactly where that site is too flat to be assigned (6 there, 1 here)."""
    excluded = [name for a, b, name, _, _ in law2 if K.fold_made_twins(a) or K.fold_made_twins(b)]
    kept = [(name, key, strict) for a, b, name, key, strict in law2 if name not in excluded]
    assert sorted({name.split(" ")[1] for name in excluded}) == ["188", "209", "21", "226", "30", "89"] and len(excluded) == LAW2_FOLD_TWINS
    for name, key, strict in kept:
        assert key["verdict"] == strict["verdict"], name
        assert key["sites"] == strict["sites"], name
    for a, b, name, key, strict in law2:
        if name in excluded and key["verdict"] != strict["verdict"]:
            assert (key["verdict"], strict["verdict"]) == (K.IDENTICAL, K.UNASSIGNED), name
    assert len(kept) == LAW2_PAIRS >= 100
    assert {key["verdict"] for _, key, _ in kept} == {K.DIFFERENT, K.IDENTICAL, K.MIRROR, K.STEREOISOMER, K.UNASSIGNED}


# ------------------------------------------------------------------------------------------------------------------ f. law 3

LAW3_FORMS, LAW3_BROKEN = 75, ["corpus 212"]     # counted on the CPU with the mirror alone: 1 of 75 = 1.3 %


def test_law_3_a_single_shift_changes_nothing():
    """For every molecule m of the corpus and every single shifted form s of it (positions kept): compare(s, m) = compare(m, m) and
    compare(reflected(s), m) = compare(reflected(m), m).  The one-pass normalisation (deviation of diffspectra_mobile.h) can break this
    where the shift changes the set of paths; such cases are counted, listed and excluded - a condition, not a measurement: at most 5 %."""
    forms = K.shifted_forms()
    broken = []
    for k, path, m, s in forms:
        first = K.compare(s, m)["verdict"] == K.compare(m, m)["verdict"]
        second = K.compare(K.reflected(s), m)["verdict"] == K.compare(K.reflected(m), m)["verdict"]
        if not (first and second):
            broken.append(f"corpus {k}")
    assert len(forms) == LAW3_FORMS
    assert sorted(set(broken)) == LAW3_BROKEN
    assert len(broken) <= 0.05 * len(forms)
    # the corpus is small molecules: few of its shifted forms have a site at all (counted: 2), so the law is also run on the hand molecules
    # that have both a mobile group and a site, every shift of every path, where it must hold without exception
    assert sum(1 for _, _, m, _ in forms if K.Perception(m).tetra or K.Perception(m).ez) == 2
    ran = 0
    for name in ("lactic acid", "alanine", "4-(1-fluoroethyl)imidazole", "5-(1-fluoroethyl)imidazole", "(E)-crotonic acid", "(Z)-crotonic acid", "fumaric acid",
                 "maleic acid"):
        m = MOLS[name]
        rec, n = SM.records([m])
        for path in MM.Analysis(rec[0], n[0]).paths:
            s = MM.shifted(m, path)
            assert K.compare(s, m)["verdict"] == K.compare(m, m)["verdict"] == K.IDENTICAL, name
            assert K.compare(K.reflected(s), m)["verdict"] == K.compare(K.reflected(m), m)["verdict"], name
            assert K.compare(m, m)["sites"][0] + K.compare(m, m)["sites"][1] >= 1
            ran += 1
    assert ran >= 8


# ------------------------------------------------------------------------------------------------------------------ g. thresholds

def test_no_site_of_the_seeded_sets_sits_on_a_threshold(law2):
    margins = [key["margin"] for _, _, _, key, _ in law2] + [K.Perception(x).margin for _, _, m, s in K.shifted_forms() for x in (m, s)]
    margins += [K.Perception(m).margin for m in MOLS.values()]
    assert min(margins) > 1e-6, min(margins)


# ------------------------------------------------------------------------------------------------------------------ rows without an answer

def test_budget_rows_and_unusable_rows_are_defined():
    mol = MM.named("2-pyridone")
    mol = dict(mol, pos=np.zeros((len(mol["type"]), 3)))
    need = K.Perception(mol).nodes
    assert need > MM.analyse(*[x[0] for x in SM.records([mol])])["nodes"] > 0, "the site search goes on where the group search stops"
    assert K.site_rows(mol, max_nodes=need)["status"] == K.OK
    short = K.site_rows(mol, max_nodes=need - 1)
    assert short["status"] == K.ROW_UNDECIDED and short["nodes"] == 0 and not short["site"][:, 0].any() and set(short["site"][:, 1]) == {K.NO_PARTNER}
    assert short["masks"] == [0] * 9 and not short["volume"].any()
    assert K.compare(mol, mol, max_nodes=need - 1)["verdict"] == K.UNDECIDED
    bad = dict(mol, type=np.where(np.arange(len(mol["type"])) == 0, 5, mol["type"]))
    assert K.site_rows(bad)["status"] == K.UNUSABLE and K.compare(bad, mol)["verdict"] == K.INVALID
