"""GPU: ``dsb_brics_records`` and ``dsb_brics_fragment_records`` (csrc/ds_brics.hip) and what ``structure_metrics`` and ``evaluate`` build on them
against the plain-Python mirror of tests/brics_mirror.py, which is written from include/diffspectra_brics.h and pinned to hand-stated
expectations by tests/test_brics_cpu.py.  Every output is an integer or a byte and is compared exactly; the one float, ``frag``, is the same
Python expression on the same integers on both sides and is compared with ``==``."""
import math

import numpy as np
import pytest
import torch

from diffspectra_amd import engine as E, shard, structure_metrics as S
from tests import brics_mirror as B, graph_mirror as GM, scaffold_mirror as K, structure_mirror as SM
from tests.helpers import to_dev
from tests.test_scaffold_cpu import same_partition
from tests.test_valence_gpu import random_records

pytestmark = pytest.mark.gpu

GUARD_ROWS = 3
PLAIN = ("frag", "n_generated", "n_test", "fragments_generated", "fragments_test", "distinct_generated", "distinct_test", "shared", "mean_cuts")


def on(dev, rec, n):
    return to_dev(dev, rec, torch.uint8), to_dev(dev, n, torch.int32)


def gpu_arrays(dev, rec, n):
    """``brics_records`` as the five numpy arrays of ``brics_mirror.as_arrays``."""
    out = [t.cpu() for t in E.brics_records(*on(dev, rec, n))]
    assert [t.dtype for t in out] == [torch.int32, torch.uint8, torch.uint8, torch.int32, torch.uint8]
    assert [tuple(t.shape) for t in out] == [(len(n), 29), (len(n), 28, 4), (len(n), 29), (len(n), 4), (len(n),)]
    return [t.numpy() for t in out]


def same_arrays(got, want, keys=B.KEYS):
    for key, g, w in zip(keys, got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (key, g.shape, w.shape, g.dtype, w.dtype)
        rows = np.nonzero((g != w).reshape(len(g), -1).any(1))[0]
        assert rows.size == 0, (key, rows[:5].tolist(), g[rows[0]].tolist(), w[rows[0]].tolist())


def gpu_fragments(dev, rec, n, aromatic=True):
    out = S.brics_fragment_records(*on(dev, rec, n), aromatic=aromatic)
    assert [t.dtype for t in out] == [torch.uint8, torch.int32, torch.int64, torch.uint8]
    return [t.cpu().numpy() for t in out]


FRAGMENT_KEYS = ("out_rec", "out_n", "out_owner", "out_source")


@pytest.fixture(scope="module")
def molecules():
    """The table, three renumberings of each of its molecules (with the permutations), the Kekule pairs and the derived set as one record
    table, with the mirror's rows: computed once, shared, never changed."""
    rows = B.hand_table()
    rng = np.random.default_rng(23)
    table = [mol for _, mol, _ in rows]
    perms, renumbered = [], []
    for mol in table:
        for _ in range(3):
            perm = rng.permutation(len(mol["type"]))                            # new atom i is old atom perm[i]
            perms.append(perm)
            renumbered.append(B.renumbered(mol, perm))
    kekule = [m for _, a, b in B.kekule_pairs() for m in (a, b)]
    derived = B.derived_set()
    rec, n = SM.records(table + renumbered + kekule + derived)
    return dict(rows=rows, perms=perms, rec=rec, n=n, want=B.analyse_table(rec, n), kekule=slice(len(table) * 4, len(table) * 4 + len(kekule)),
                derived=slice(len(n) - len(derived), len(n)))


# ------------------------------------------------------------------------------------------------------------------ the kernels

def test_table_renumberings_and_derived_set_against_the_mirror(gpu_device, molecules):
    rows, perms, rec, n, want = (molecules[k] for k in ("rows", "perms", "rec", "n", "want"))
    got = gpu_arrays(gpu_device, rec, n)
    same_arrays(got, B.as_arrays(want))
    # ... and so the hand-stated table holds for the kernel, under renumbering too
    T = len(rows)
    cuts_of = lambda p: [tuple(c) for c in got[1][p].tolist() if c != [0xff] * 4]
    for k, (name, mol, cuts) in enumerate(rows):
        assert cuts_of(k) == sorted(cuts) and got[3][k, 1] == len(cuts) and got[4][k] == 0, name
        for j in range(3):
            assert cuts_of(T + 3 * k + j) == B.moved_cuts(cuts, perms[3 * k + j]), name
    # the ground the comparison stands on (asserted on the mirror in tests/test_brics_cpu.py)
    part = got[3][molecules["derived"]]
    assert len(part) >= 250 and int((part[:, 1] == 0).sum()) >= 40 and int((part[:, 1] >= 2).sum()) >= 40
    labels = got[1][molecules["derived"]][:, :, 2:].reshape(-1)
    assert all(int((labels == label).sum()) >= 5 for label in B.LABELS)
    # the header's invariant, with the components as dsq_match_records counts them: fragments = components + cuts
    components = E.substructure_records(*on(gpu_device, rec, n), torch.zeros(0, E.PATTERN_WORDS, dtype=torch.int32, device=gpu_device))[5].cpu().numpy()
    assert np.array_equal(got[3][:, 2], components + got[3][:, 1]) and int(components.max()) >= 2


@pytest.mark.parametrize("aromatic", [True, False])
def test_fragment_records_against_the_mirror(gpu_device, molecules, aromatic):
    rec, n = molecules["rec"], molecules["n"]
    got = gpu_fragments(gpu_device, rec, n, aromatic)
    want = B.fragment_table(rec, n, aromatic)
    same_arrays(got, want, FRAGMENT_KEYS)
    assert len(got[1]) == sum(w["summary"][2] for w in molecules["want"]) and int(got[1].max()) <= 29
    bonds = got[0][:, SM.BOND:SM.BOND_END]
    assert int(got[0][:, SM.TYPE:SM.FC].max()) == B.ATTACH_TYPE and int(bonds.max()) == (B.AROMATIC_ORDER if aromatic else 3) and not got[0][:, SM.BOND_END:].any()
    sym = bonds.reshape(-1, 29, 29)
    assert np.array_equal(sym, sym.transpose(0, 2, 1))                          # written symmetrically


def test_kekule_drawings_with_and_without_the_aromatic_byte(gpu_device, molecules):
    """The two drawings of every Kekule pair: the same cuts; one set of fragment classes with the aromatic byte, two without."""
    rec, n = molecules["rec"][molecules["kekule"]], molecules["n"][molecules["kekule"]]
    rec_d, n_d = on(gpu_device, rec, n)
    for aromatic in (True, False):
        f_rec, f_n, owner, _ = S.brics_fragment_records(rec_d, n_d, aromatic=aromatic)
        cls = S.graph_classes(f_rec, f_n).cpu().numpy()
        owner = owner.cpu().numpy()
        for pair in range(len(n) // 2):
            a, b = sorted(cls[owner == 2 * pair].tolist()), sorted(cls[owner == 2 * pair + 1].tolist())
            assert len(a) == len(b) >= 2 and (a == b) == aromatic, (pair, aromatic, a, b)
    with_byte, with_orders = (gpu_fragments(gpu_device, rec, n, aromatic) for aromatic in (True, False))
    differ = with_byte[0] != with_orders[0]
    assert differ.any() and set(with_byte[0][differ].tolist()) == {B.AROMATIC_ORDER} and set(with_orders[0][differ].tolist()) == {1, 2}
    assert all(np.array_equal(a, b) for a, b in zip(with_byte[1:], with_orders[1:]))


def ring_of(k, start=0):
    return [(start + i, start + (i + 1) % k) for i in range(k)]


def polyether_29():
    """29 heavy atoms, C C (O C C) x 9: every C-O bond is a 3-4 cut, 18 cuts and 19 fragments - the most the rules give on a chain."""
    types = [1, 1] + [3, 1, 1] * 9
    return GM.molecule(types, [(i, i + 1) for i in range(28)])


def with_garbage(rng, rec, n):
    """``rec`` with random bytes in everything the contract ignores: atoms >= n (n clamped), the lower triangle and the diagonal, bond bytes with
    an end >= n, the pad."""
    P = len(n)
    atom = np.arange(29)[None, :] < np.clip(n, 0, 29)[:, None]
    pair = np.triu(np.ones((29, 29), bool), 1)[None] & atom[:, :, None] & atom[:, None, :]
    ignored = np.zeros((P, SM.RECORD_BYTES), bool)
    ignored[:, SM.POS:SM.TYPE] = np.repeat(~atom, 12, axis=1)
    ignored[:, SM.TYPE:SM.FC] = ignored[:, SM.FC:SM.BOND] = ~atom
    ignored[:, SM.BOND:SM.BOND_END] = (~pair).reshape(P, -1)
    ignored[:, SM.BOND_END:] = True
    out = rec.copy()
    out[ignored] = rng.integers(0, 256, size=int(ignored.sum()), dtype=np.uint8)
    return out


def test_sizes_garbage_and_the_hard_shapes(gpu_device, molecules):
    rng = np.random.default_rng(20261020)
    # random bytes everywhere: n of 1, 2, 28, 29 and two clamped counts; usable and unusable rows, dense graphs (such records have no cut)
    sizes = np.array([1, 2, 28, 29, 28, 29, 40, -3] * 30, np.int32)
    rec, n, clean = random_records(rng, len(sizes), garbage=True, sizes=sizes)
    want = B.analyse_table(rec, n)
    got = gpu_arrays(gpu_device, rec, n)
    same_arrays(got, B.as_arrays(want))
    assert {w["status"] for w in want} == {B.OK, B.UNUSABLE} and sum(w["summary"][2] > 1 for w in want) > 50
    same_arrays(gpu_arrays(gpu_device, clean, n), got)                           # what is ignored is ignored
    for aromatic in (True, False):
        frags = gpu_fragments(gpu_device, rec, n, aromatic)
        same_arrays(frags, B.fragment_table(rec, n, aromatic), FRAGMENT_KEYS)
        same_arrays(gpu_fragments(gpu_device, clean, n, aromatic), frags, FRAGMENT_KEYS)
    # molecules with cuts, garbage in what is ignored: every third record of the shared table, the 28- and 29-atom ones of the derived set
    # and polyethers of 28 and 29 atoms, the 29-atom ones with their count given as 40
    big = np.nonzero(molecules["n"] >= 28)[0]
    ether = polyether_29()
    ether_28 = GM.molecule(ether["type"][:28], [(i, i + 1) for i in range(27)])
    e_rec, e_n = SM.records([ether, ether_28, GM.permuted(ether, rng), GM.permuted(ether_28, rng)])
    rows = np.concatenate([np.arange(0, len(molecules["n"]), 3), big])
    rec, n = np.concatenate([molecules["rec"][rows], e_rec]), np.concatenate([molecules["n"][rows], e_n])
    assert (n == 28).sum() >= 3 and (n == 29).sum() >= 3
    n[n == 29] = 40
    dirty = with_garbage(rng, rec, n)
    want = B.analyse_table(dirty, n)
    got = gpu_arrays(gpu_device, dirty, n)
    same_arrays(got, B.as_arrays(want))
    same_arrays(gpu_arrays(gpu_device, rec, n), got)
    assert sum(w["summary"][1] > 0 for w in want) > 80 and not np.array_equal(dirty, rec)
    for aromatic in (True, False):
        frags = gpu_fragments(gpu_device, dirty, n, aromatic)
        same_arrays(frags, B.fragment_table(dirty, n, aromatic), FRAGMENT_KEYS)
        same_arrays(gpu_fragments(gpu_device, rec, n, aromatic), frags, FRAGMENT_KEYS)
    # the 29-atom chain, the 29-ring, the complete graph, the polyether (18 cuts, the most the rules give on a chain) and sparse 29-atom graphs
    chain = GM.carbons(29, [(i, i + 1) for i in range(28)])
    big_ring = GM.carbons(29, ring_of(29))
    sparse = [GM.random_molecule(rng, 29) for _ in range(20)]
    hard = [GM.k29(), chain, big_ring, ether, GM.permuted(ether, rng), GM.permuted(chain, rng)]
    rec, n = SM.records(hard + sparse)
    rec[0, SM.BOND_END:] = 0xEE
    rec[0, SM.BOND:SM.BOND_END].reshape(29, 29)[np.tril_indices(29)] = 0xEE      # garbage in the lower triangle and on the diagonal
    want = B.analyse_table(rec, n)
    got = gpu_arrays(gpu_device, rec, n)
    same_arrays(got, B.as_arrays(want))
    assert got[3][:6].tolist() == [[29, 0, 1, 29], [29, 0, 1, 29], [29, 0, 1, 29], [29, 18, 19, 2], [29, 18, 19, 2], [29, 0, 1, 29]]
    assert got[1][3, :18, 2:].tolist() == [[4, 3], [3, 4]] * 9 and (got[1][3, 18:] == 0xff).all() and got[2][3].tolist() == [0, 0] + [k for f in range(1, 19, 2) for k in (f, f + 1, f + 1)]
    for aromatic in (True, False):
        same_arrays(gpu_fragments(gpu_device, rec, n, aromatic), B.fragment_table(rec, n, aromatic), FRAGMENT_KEYS)


def test_every_kind_of_unusable_record(gpu_device, molecules):
    names = [name for name, *_ in molecules["rows"]]
    k = names.index("ethyl acetate")
    count = int(molecules["n"][k])
    assert count == 14
    base, n = np.repeat(molecules["rec"][k:k + 1], 7, axis=0), np.full(7, count, np.int32)
    n[2] = 0
    base[0, SM.TYPE + count - 1] = 5                                            # a type byte above 4 (the last atom)
    base[1, SM.BOND + 3 * 29 + 12] = 4                                          # a bond byte above 3, upper triangle
    n[3] = -7                                                                   # clamped to 0
    base[4, SM.BOND + 12 * 29 + 3] = 4                                          # the same pair in the lower triangle: not looked at
    base[5, SM.BOND + 28 * 29 + 28] = 9                                         # the diagonal: not looked at
    base[6, SM.TYPE + count] = 77                                               # an atom >= n: not looked at
    base[6, SM.BOND + 2 * 29 + count + 1] = 200
    got = gpu_arrays(gpu_device, base, n)
    same_arrays(got, B.as_arrays(B.analyse_table(base, n)))
    assert got[4].tolist() == [3, 3, 3, 3, 0, 0, 0] and not got[0][:4].any() and not got[3][:4].any() and (got[1][:4] == 0xff).all() and (got[2][:4] == 0xff).all()
    assert all(np.array_equal(a[4:], np.repeat(b[k:k + 1], 3, axis=0)) for a, b in zip(got, B.as_arrays(molecules["want"])))
    frags = gpu_fragments(gpu_device, base, n)                                   # an unusable record has no fragment
    same_arrays(frags, B.fragment_table(base, n), FRAGMENT_KEYS)
    assert frags[2].tolist() == [4] * 3 + [5] * 3 + [6] * 3


def test_guarded_outputs_repeat_runs_and_batch_independence(gpu_device, molecules):
    """Every output of both kernels between guard rows filled with a pattern (P = 65: a workgroup with three waves that have no record; F =
    the fragment total plus the guards); a ``first`` outside [0, F) writes nothing; two runs bit-identical; a row's outputs do not depend on
    the batch around it."""
    rng = np.random.default_rng(9)
    P = 65
    rows = rng.permutation(len(molecules["n"]))[:P]
    rec_d, n_d = on(gpu_device, molecules["rec"][rows], molecules["n"][rows])
    lib, stream = E.load_library(), torch.cuda.current_stream().cuda_stream

    def guarded(count, width, dtype):
        raw = torch.full((count + 2 * GUARD_ROWS, width), 0x5A, dtype=torch.uint8, device=gpu_device).view(dtype)
        return raw, raw[GUARD_ROWS:GUARD_ROWS + count]

    def intact(raw):
        b = raw.view(torch.uint8)
        return bool((b[:GUARD_ROWS] == 0x5A).all()) and bool((b[-GUARD_ROWS:] == 0x5A).all())
    bufs = [guarded(P, 29 * 4, torch.int32), guarded(P, 28 * 4, torch.uint8), guarded(P, 29, torch.uint8), guarded(P, 16, torch.int32), guarded(P, 1, torch.uint8)]
    st = lib.dsb_brics_records(rec_d.data_ptr(), n_d.data_ptr(), P, *(view.data_ptr() for _, view in bufs), stream)
    torch.cuda.synchronize()
    assert st == 0 and all(intact(raw) for raw, _ in bufs)
    plain, again = E.brics_records(rec_d, n_d), E.brics_records(rec_d, n_d)
    assert all(torch.equal(view.reshape(t.shape), t) and torch.equal(t, u) for (_, view), t, u in zip(bufs, plain, again))
    assert [molecules["want"][r]["summary"][1] for r in rows] == plain[3][:, 1].cpu().tolist()
    for sub in ([64], [5], [17, 64, 5, 0]):
        idx = torch.tensor(sub, device=gpu_device)
        alone = E.brics_records(rec_d[idx].contiguous(), n_d[idx].contiguous())
        assert all(torch.equal(s, t[idx]) for s, t in zip(alone, plain))
    assert [a.shape[0] for a in gpu_arrays(gpu_device, molecules["rec"][:0], molecules["n"][:0])] == [0] * 5
    # the fragment kernel: the rows start GUARD_ROWS into buffers of F = total + 2 * GUARD_ROWS rows
    counts = plain[3][:, 2].to(torch.int64)
    total = int(counts.sum())
    first = (torch.cumsum(counts, 0) - counts).contiguous()
    F = total + 2 * GUARD_ROWS
    outs = [guarded(total, E.RECORD_BYTES, torch.uint8), guarded(total, 4, torch.int32), guarded(total, 8, torch.int64), guarded(total, 29, torch.uint8)]
    shifted = first + GUARD_ROWS
    st = lib.dsb_brics_fragment_records(rec_d.data_ptr(), n_d.data_ptr(), P, shifted.data_ptr(), F, 1, *(raw.data_ptr() for raw, _ in outs), stream)
    torch.cuda.synchronize()
    assert st == 0 and all(intact(raw) for raw, _ in outs)
    frags, frags_again = E.brics_fragment_records(rec_d, n_d, first, total), E.brics_fragment_records(rec_d, n_d, first, total)
    assert all(torch.equal(view.reshape(t.shape), t) and torch.equal(t, u) for (_, view), t, u in zip(outs, frags, frags_again))
    same_arrays([t.cpu().numpy() for t in frags], B.fragment_table(molecules["rec"][rows], molecules["n"][rows]), FRAGMENT_KEYS)
    # a first outside [0, F): the fragments of the odd records point below 0 or at and beyond F and are not written; F = 0 writes nothing
    away = first.clone()
    away[1::4], away[3::4] = -1000, total
    outs = [guarded(total, E.RECORD_BYTES, torch.uint8), guarded(total, 4, torch.int32), guarded(total, 8, torch.int64), guarded(total, 29, torch.uint8)]
    st = lib.dsb_brics_fragment_records(rec_d.data_ptr(), n_d.data_ptr(), P, away.data_ptr(), total, 1, *(view.data_ptr() for _, view in outs), stream)
    torch.cuda.synchronize()
    assert st == 0 and all(intact(raw) for raw, _ in outs)
    written = (frags[2] % 2 == 0)                                                # by owner
    for (_, view), t in zip(outs, frags):
        assert torch.equal(view.reshape(t.shape)[written], t[written]) and bool((view.view(torch.uint8)[~written] == 0x5A).all())
    assert int((~written).sum()) > 20 and int(written.sum()) > 20
    st = lib.dsb_brics_fragment_records(rec_d.data_ptr(), n_d.data_ptr(), P, first.data_ptr(), 0, 1, *(view.data_ptr() for _, view in outs), stream)
    torch.cuda.synchronize()
    assert st == 0 and all(intact(raw) for raw, _ in outs) and bool((outs[0][1][~written] == 0x5A).all())
    # a record alone gives the rows it gives in its batch
    for p in (64, 5):
        alone = S.brics_fragment_records(rec_d[p:p + 1].contiguous(), n_d[p:p + 1].contiguous())
        mine = frags[2] == p
        assert torch.equal(alone[0], frags[0][mine]) and torch.equal(alone[1], frags[1][mine]) and torch.equal(alone[3], frags[3][mine])


def test_graph_hash_and_identity_on_fragment_bytes(gpu_device, molecules):
    """What fragment identity rests on: ``ds_graph_hash_records`` and ``ds_graph_identity_records`` compare raw type, charge and bond bytes, so
    records with type byte 5 and bond byte 4 are hashed and compared like any other - against ``graph_mirror``."""
    rng = np.random.default_rng(41)
    rec, n = molecules["rec"][molecules["derived"]][::4], molecules["n"][molecules["derived"]][::4]
    f_rec, f_n, _, _ = B.fragment_table(rec, n, True)
    assert (f_rec[:, SM.TYPE:SM.FC] == B.ATTACH_TYPE).any(1).sum() >= 50 and (f_rec[:, SM.BOND:SM.BOND_END] == B.AROMATIC_ORDER).any(1).sum() >= 10
    mols = [SM.mol_from_record(r, k) for r, k in zip(f_rec, f_n)]
    moved = [GM.permuted(m, rng) for m in mols]
    other = [mols[int(j)] for j in rng.permutation(len(mols))]
    a_rec, a_n = on(gpu_device, *SM.records(mols + mols))
    b_rec, b_n = on(gpu_device, *SM.records(moved + other))
    assert bool((a_rec[:len(mols)] == to_dev(gpu_device, f_rec, torch.uint8))[:, SM.TYPE:].all())           # the packer keeps the bytes
    hashes = E.graph_hash_records(b_rec, b_n).cpu().tolist()
    assert [h & GM.MASK for h in hashes] == [GM.graph_hash(m) for m in moved + other]
    assert [h & GM.MASK for h in E.graph_hash_records(a_rec, a_n).cpu().tolist()][:len(mols)] == [h & GM.MASK for h in hashes[:len(mols)]]
    verdict = E.graph_identity_records(a_rec, a_n, b_rec, b_n)[0].cpu().tolist()
    stated = [int(GM.same_graph(x, y)) for x, y in zip(mols + mols, moved + other)]
    assert verdict == stated and verdict[:len(mols)] == [1] * len(mols) and 0 < sum(stated[len(mols):]) < len(mols)


# ------------------------------------------------------------------------------------------------------------------ the public interface

@pytest.fixture(scope="module")
def two_sets(molecules):
    """Two disjoint halves of the derived set plus 28 molecules that both get."""
    rec, n = molecules["rec"][molecules["derived"]], molecules["n"][molecules["derived"]]
    shared = np.arange(5, 285, 10)
    rest = np.setdiff1d(np.arange(len(n)), shared)
    gen, test = np.concatenate([rest[0::2], shared]), np.concatenate([rest[1::2], shared])
    return (rec[gen], n[gen]), (rec[test], n[test])


def test_brics_and_the_fragment_metric_against_the_mirror(gpu_device, molecules, two_sets):
    rec, n, want = molecules["rec"], molecules["n"], molecules["want"]
    found = S.brics(to_dev(gpu_device, rec, torch.uint8), n.tolist())
    assert isinstance(found, S.Brics) and found.env.device.type == gpu_device.type and bool(found.usable.all())
    assert found.n_cuts.cpu().tolist() == [w["summary"][1] for w in want] and found.n_fragments.cpu().tolist() == [w["summary"][2] for w in want]
    gen, test = two_sets
    gen_d, test_d = on(gpu_device, *gen), on(gpu_device, *test)
    same = lambda mine, stated: {k: mine[k] for k in PLAIN} == {k: stated[k] for k in PLAIN}
    for aromatic in (True, False):
        stated = B.fragment_metric(gen, test, aromatic)
        assert stated["distinct_generated"] >= 30 and stated["distinct_test"] >= 30 and stated["shared"] >= 10 and 0.0 < stated["frag"] < 1.0
        fn = S.get_fragment_metric(test_d, unique=False, aromatic=aromatic)
        mine = fn(gen_d)
        assert set(mine) == set(stated) and isinstance(mine["frag"], float) and mine["fragment_class"].dtype == torch.int64
        assert same(mine, stated), ({k: mine[k] for k in PLAIN}, {k: stated[k] for k in PLAIN})
        assert mine["owner"].cpu().tolist() == stated["owner"] and same_partition(mine["fragment_class"].cpu().tolist(), stated["fragment_class"])
    # a keep mask, with the same test side (Kekule orders)
    keep = np.arange(len(gen[1])) % 3 != 0
    stated = B.fragment_metric((gen[0][keep], gen[1][keep]), test, False)
    mine = fn(gen_d, keep=to_dev(gpu_device, keep, torch.bool))
    assert same(mine, stated) and mine["n_generated"] == int(keep.sum())
    # one representative per class of molecules on both sides
    gu, tu = K.unique_rows(*gen), K.unique_rows(*test)
    stated = B.fragment_metric((gen[0][gu], gen[1][gu]), (test[0][tu], test[1][tu]))
    mine = S.get_fragment_metric(test_d)(gen_d)
    assert same(mine, stated) and mine["n_generated"] == len(gu) <= len(gen[1]) and 0.0 < mine["frag"] < 1.0
    # an empty generated side
    none = fn(gen_d, keep=torch.zeros(len(gen[1]), dtype=torch.bool, device=gpu_device))
    assert math.isnan(none["frag"]) and math.isnan(none["mean_cuts"]) and none["fragments_generated"] == 0 and none["fragment_class"].numel() == 0


# ------------------------------------------------------------------------------------------------------------------ evaluation

def test_evaluate_reports_the_fragments(gpu_device, tmp_path, monkeypatch):
    """diffspectra_evaluate(structure_metrics=True) on filler weights, 3 steps, K = 2: with ``cfg.eval.fragments`` the 'structure' dict holds the
    entry, equal to the mirror on the run's records; without the flag it has no such key."""
    from diffspectra_amd import filler, evaluate as EV
    from diffspectra_amd.config import qm9s_config
    from diffspectra_amd.dataset_pack import PackedSpectraTable
    from diffspectra_amd.registry import create_model
    from tests.test_structure_metrics_gpu import _graph_dataset
    import diffspectra_amd.dmt  # noqa: F401
    K_, T = 2, 3
    cfg = qm9s_config("ir", device=gpu_device, steps=3, batch_size=4, num_samples=T)
    cfg.eval.begin_ckpt, cfg.eval.end_ckpt, cfg.eval.ckpts, cfg.eval.top_k = 40, 40, "", K_
    table = PackedSpectraTable.from_dataset(_graph_dataset(8, seed=21), "ir", device=gpu_device)
    donor = create_model(cfg)
    donor.eval()
    filler.fill_module_(donor)
    ema = EV.ExponentialMovingAverage(donor.parameters(), decay=0.999)
    (tmp_path / "checkpoints").mkdir()
    EV.save_checkpoint(str(tmp_path / "checkpoints" / "checkpoint_40.pth"), dict(optimizer=None, model=donor, ema=ema, step=7))
    gather, kept = shard.gather_by_slot, []

    def gather_and_keep(rec, n_atoms):
        kept.append(gather(rec, n_atoms))
        return kept[-1]
    torch.manual_seed(42)
    plain = EV.diffspectra_evaluate(cfg, str(tmp_path), table, structure_metrics=True)[40]["metrics"]["structure"]
    assert "fragments" not in plain
    cfg.eval.fragments = True
    monkeypatch.setattr(shard, "gather_by_slot", gather_and_keep)
    torch.manual_seed(42)
    res = EV.diffspectra_evaluate(cfg, str(tmp_path), table, structure_metrics=True)[40]
    monkeypatch.setattr(shard, "gather_by_slot", gather)
    st = res["metrics"]["structure"]
    assert set(st) == set(plain) | {"fragments"}
    fr = st["fragments"]
    assert set(fr) == set(PLAIN) | {"fragment_class", "owner"}
    gen_rec = kept[-1].cpu().numpy()
    gen_n = np.array([len(atom) for _, atom, _, _ in res["processed_mols"]], np.int32)
    gt_rec, gt_n = table.gt_records.cpu().numpy(), table.num_atom.numpy()
    gu, tu = K.unique_rows(gen_rec, gen_n), K.unique_rows(gt_rec, gt_n)
    stated = B.fragment_metric((gen_rec[gu], gen_n[gu]), (gt_rec[tu], gt_n[tu]))
    same_float = lambda a, b: a == b or (a != a and b != b)
    assert all(fr[k] == stated[k] for k in PLAIN if k not in ("frag", "mean_cuts")), (fr, stated)
    assert same_float(fr["frag"], stated["frag"]) and same_float(fr["mean_cuts"], stated["mean_cuts"])
    assert fr["owner"].cpu().tolist() == stated["owner"] and same_partition(fr["fragment_class"].cpu().tolist(), stated["fragment_class"])
    assert fr["n_test"] == len(tu) and fr["fragments_test"] >= len(tu)
