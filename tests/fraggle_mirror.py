"""CPU yardstick of ``dsf_fraggle_fragmentations``, ``dsf_path_fingerprints`` and ``dsf_fraggle_similarity_records`` in plain Python, written from
the text of include/diffspectra_fraggle.h and not from the kernel: the bond sets by the ESU enumeration on the line graph, the bond codes and
the hash, the per-atom bits, the four kinds of fragmentation with their integer thresholds, the marking with its ring step and the best
Tanimoto by cross-multiplication.  The graph perception (the fold, ring bonds, aromatic cycles, the bond classes) is that of
tests/substructure_mirror.py, as the header refers to diffspectra_substructure.h for it.  It works on raw record bytes, so whatever the
contract says is ignored can hold garbage.

Also here: the hand-stated table of molecules with their fragmentations (the pin: RDKit cannot run where the project runs) and the seeded
derived set of pairs that the CPU test checks for coverage and the GPU test compares on.
"""
from __future__ import annotations

import functools
import itertools

import numpy as np

from tests import brics_mirror as B, graph_mirror as GM, groups_mirror as G, structure_mirror as SM, substructure_mirror as Q, valence_mirror as VM

OK, UNDECIDED, UNUSABLE, INVALID = 0, 1, 2, 3
W = SM.W
MAX_NODES, DEFAULT_NODES, MAX_BONDS, MAX_PATH = 1 << 20, 1 << 15, 60, 5
FP_BITS, FP_WORDS = 1024, 32
CODE_ATTACH, CODE_WILD, CODE_WILD_AROMATIC = 10, 12, 13
NO_CUT, MAX_FRAGMENTATIONS, TRUNCATED = 1023, 256, 1 << 30
MASK64 = (1 << 64) - 1
H = 0


# ------------------------------------------------------------------------------------------------------------------ the fingerprint

def fmix(x):
    x ^= x >> 30
    x = (x * 0xbf58476d1ce4e5b9) & MASK64
    x ^= x >> 27
    x = (x * 0x94d049bb133111eb) & MASK64
    return x ^ (x >> 31)


def mix2(a, b):
    return fmix((a + 0x9e3779b97f4a7c15 * (b + 1)) & MASK64)


@functools.lru_cache(maxsize=None)
def set_bits(codes):
    """The two bits (as one 1024-bit int) of a bond set with the ascending bond codes ``codes``."""
    h = len(codes)
    for c in codes:
        h = mix2(h, c)
    return (1 << (h & 1023)) | (1 << ((h >> 32) & 1023))


class Over(Exception):
    pass


def bond_sets(ends, limit, roots=None):
    """Every connected set of 1..5 of the bonds ``ends`` = [(a, b)] as a tuple of bond numbers, each exactly once: the set with lowest bond e
    is grown from e by adjacent higher bonds that no earlier member could have added.  Raises Over once there are more than ``limit``.
    ``roots``: the order in which the lowest bonds are taken (the verdict does not depend on it)."""
    inc = {}
    for e, (a, b) in enumerate(ends):
        inc[a] = inc.get(a, 0) | 1 << e
        inc[b] = inc.get(b, 0) | 1 << e
    near = [(inc[a] | inc[b]) & ~(1 << e) for e, (a, b) in enumerate(ends)]
    out = []

    def add(s):
        out.append(s)
        if len(out) > limit:
            raise Over

    def grow(sub, ext, closed, above):
        while ext:
            w = (ext & -ext).bit_length() - 1
            ext &= ext - 1
            new = sub + (w,)
            add(new)
            if len(new) < MAX_PATH:
                grow(new, ext | (near[w] & ~closed & above), closed | near[w], above)

    for e in (range(len(ends)) if roots is None else roots):
        add((e,))
        grow((e,), near[e] & ~((2 << e) - 1), near[e] | 1 << e, ~((2 << e) - 1))
    return out


class Fingerprint:
    """The fingerprint of a graph with the bonds [(a, b, class)] and the atom codes {atom: code}: ``count`` bond sets, ``fp`` (a 1024-bit
    int), ``atom_bits`` {atom: int}; ``over`` when the count is beyond ``max_nodes`` (then nothing else is set).  ``recoded(code)`` gives the
    fingerprint word of the same graph under other atom codes."""

    def __init__(self, bonds, code, max_nodes, atoms=True):
        self.over = len(bonds) > MAX_BONDS + 1                                   # a fragment graph may have one bond more than its record
        self.fp, self.atom_bits, self.count = 0, {}, -1
        if not self.over:
            try:
                sets = bond_sets([(a, b) for a, b, _ in bonds], max_nodes)
            except Over:
                self.over = True
        if self.over:
            return
        self.count = len(sets)
        self.shapes = []                                                         # per set: ((a, degree of a, b, degree of b, class), ...)
        for s in sets:
            deg = {}
            for e in s:
                a, b, _ = bonds[e]
                deg[a] = deg.get(a, 0) + 1
                deg[b] = deg.get(b, 0) + 1
            self.shapes.append(tuple((bonds[e][0], deg[bonds[e][0]], bonds[e][1], deg[bonds[e][1]], bonds[e][2]) for e in s))
        for shape in self.shapes:
            bits = self._bits(shape, code)
            self.fp |= bits
            if atoms:
                for a, _, b, _, _ in shape:
                    self.atom_bits[a] = self.atom_bits.get(a, 0) | bits
                    self.atom_bits[b] = self.atom_bits.get(b, 0) | bits

    @staticmethod
    def _bits(shape, code):
        codes = []
        for a, da, b, db, cls in shape:
            x, y = code[a] * 8 + da, code[b] * 8 + db
            codes.append((min(x, y) << 9) | (max(x, y) << 2) | cls)
        return set_bits(tuple(sorted(codes)))

    def recoded(self, code):
        fp = 0
        for shape in self.shapes:
            fp |= self._bits(shape, code)
        return fp


def words(fp):
    """A 1024-bit int as the 32 int32 words of the kernel."""
    return np.array([(fp >> (32 * w)) & 0xFFFFFFFF for w in range(FP_WORDS)], np.uint32).view(np.int32)


def popcount(x):
    return bin(x).count("1")


# ------------------------------------------------------------------------------------------------------------------ the graph

class Mol:
    """One record as the header sees it: ``atoms`` (matchable, ascending), ``bonds`` [(a, b, class)] ascending, ``ring`` {bond number: ring
    bond}, ``code`` {atom: atom code}, ``nbrs`` {atom: set}."""

    def __init__(self, rec, n):
        g = Q.Graph(rec, n)
        self.usable = g.usable
        if not g.usable:
            return
        _, types, _, _, _, _ = VM.read(rec, n, VM.RECORD)
        self.atoms = list(g.matchable)
        self.hac = len(self.atoms)
        aromatic = set(g.aromatic)
        self.aromatic = aromatic
        self.code = {a: 2 * types[a] + int(a in aromatic) for a in self.atoms}
        self.bonds = sorted((a, b, c % 4) for (a, b), c in g.cls.items() if a < b)
        self.ring = [g.cls[a, b] >= 4 for a, b, _ in self.bonds]
        self.nbrs = {a: set() for a in self.atoms}
        for a, b, _ in self.bonds:
            self.nbrs[a].add(b)
            self.nbrs[b].add(a)
        self.over_bonds = len(self.bonds) > MAX_BONDS
        self._fp = {}

    def fingerprint(self, max_nodes):
        if max_nodes not in self._fp:
            self._fp[max_nodes] = Fingerprint(self.bonds, self.code, max_nodes) if not self.over_bonds else _OVER
        return self._fp[max_nodes]

    # ------------------------------------------------------------------------------------------------ fragmentations
    def pieces(self, cuts):
        """The components of the matchable graph without the bonds ``cuts`` = {frozenset((a, b))}, by ascending lowest atom."""
        seen, out = set(), []
        for s in self.atoms:
            if s in seen:
                continue
            seen.add(s)
            piece, stack = [], [s]
            while stack:
                u = stack.pop()
                piece.append(u)
                for v in self.nbrs[u]:
                    if v not in seen and frozenset((u, v)) not in cuts:
                        seen.add(v)
                        stack.append(v)
            out.append(sorted(piece))
        return out

    def on_cycle(self, a, piece, cuts):
        """Does atom ``a`` lie on a cycle of its piece: a neighbour is reached without the bond to it."""
        inside = set(piece)
        for g in self.nbrs[a]:
            if g not in inside or frozenset((a, g)) in cuts:
                continue
            seen, stack = {a}, [a]
            while stack:
                u = stack.pop()
                for v in self.nbrs[u]:
                    if v in seen or frozenset((u, v)) in cuts or (u == a and v == g):
                        continue
                    seen.add(v)
                    stack.append(v)
            if g in seen:
                return True
        return False

    def cut_bonds(self):
        ring_degree = {a: 0 for a in self.atoms}
        for (a, b, _), r in zip(self.bonds, self.ring):
            if r:
                ring_degree[a] += 1
                ring_degree[b] += 1
        chain = [e for e, ((a, b, c), r) in enumerate(zip(self.bonds, self.ring)) if not r and c == 0]
        ring = [e for e, ((a, b, c), r) in enumerate(zip(self.bonds, self.ring)) if r and (ring_degree[a] >= 3 or ring_degree[b] >= 3)]
        return chain, ring

    def _judge(self, cut_numbers):
        """[(piece, attachment atoms (with repeats), size)] of the cut."""
        cuts = {frozenset(self.bonds[e][:2]) for e in cut_numbers}
        ends = [x for e in cut_numbers for x in self.bonds[e][:2]]
        return cuts, [(p, [x for x in ends if x in set(p)], len(p) + sum(1 for x in ends if x in set(p))) for p in self.pieces(cuts)]

    def fragmentations(self):
        """[(kind, kept atoms, cut bond numbers, sum of the kept sizes)] in the header's order."""
        chain, ring = self.cut_bonds()
        hac, out = self.hac, []

        def terminal(cut_numbers, kind):
            _, judged = self._judge(cut_numbers)
            kept = [(p, size) for p, att, size in judged if len(att) == 1 and size > 3]
            total = sum(size for _, size in kept)
            if kept and 5 * total > 3 * hac:
                out.append((kind, sorted(a for p, _ in kept for a in p), tuple(cut_numbers), total))
        for c in chain:
            terminal([c], 0)
        for c1, c2 in itertools.combinations(chain, 2):
            terminal([c1, c2], 1)
        passed = []
        for r1, r2 in itertools.combinations(ring, 2):
            cuts, judged = self._judge([r1, r2])
            if len(judged) != 2:
                continue
            good = False
            for p, att, size in judged:
                if len(att) == 2 and all(self.on_cycle(a, p, cuts) for a in att) and size > 3 and 5 * size > 2 * hac:
                    out.append((2, p, (r1, r2), size))
                    good = True
            if good:
                passed.append((r1, r2))
        for r1, r2 in passed:
            for c in chain:
                cuts, judged = self._judge([r1, r2, c])
                kept = []
                for p, att, size in judged:
                    if len(att) == 2 and all(self.on_cycle(a, p, cuts) for a in att) and size > 3:
                        kept.append((p, size))
                    elif len(att) == 1 and size > 3:
                        kept.append((p, size))
                total = sum(size for _, size in kept)
                if len(kept) == 2 and 5 * total > 3 * hac:
                    out.append((3, sorted(a for p, _ in kept for a in p), (r1, r2, c), total))
        return out

    def fragment_graph(self, kept, cut_numbers):
        """(bonds, codes) of the fragment graph; attachment points are numbered from 100."""
        kept, cut_numbers = set(kept), set(cut_numbers)
        bonds, code, att = [], {a: self.code[a] for a in kept}, 100
        for e, (a, b, c) in enumerate(self.bonds):
            if e in cut_numbers:
                for x in (a, b):
                    if x in kept:
                        bonds.append((x, att, c))
                        code[att] = CODE_ATTACH
                        att += 1
            elif a in kept and b in kept:
                bonds.append((a, b, c))
        return bonds, code

    # ------------------------------------------------------------------------------------------------ marking
    def distances(self, start, without):
        dist, frontier = {start: 0}, [start]
        while frontier:
            nxt = []
            for u in frontier:
                for v in self.nbrs[u]:
                    if v not in dist and frozenset((u, v)) != without:
                        dist[v] = dist[u] + 1
                        nxt.append(v)
            frontier = nxt
        return dist

    def marked(self, A, max_nodes):
        """(the atoms marked against the fragment fingerprint ``A``, those of the first step alone)."""
        bits = self.fingerprint(max_nodes).atom_bits
        first = {a for a in self.atoms if bits.get(a, 0) and 5 * popcount(bits[a] & A) < 4 * popcount(bits[a])}
        marked = set(first)
        for (a, b, _), r in zip(self.bonds, self.ring):
            if not r:
                continue
            for m, x in ((a, b), (b, a)):
                if m in first:
                    dm, dx = self.distances(m, frozenset((m, x))), self.distances(x, frozenset((m, x)))
                    marked |= {v for v in dm if v in dx and dm[v] + dx[v] == dm[x]}
        return marked, first

    def marked_fp(self, marked, max_nodes):
        code = {a: (CODE_WILD_AROMATIC if a in self.aromatic else CODE_WILD) if a in marked else c for a, c in self.code.items()}
        return self.fingerprint(max_nodes).recoded(code)


class _Over:
    over, count, fp, atom_bits = True, -1, 0, {}


_OVER = _Over()


# ------------------------------------------------------------------------------------------------------------------ the entry points

def pack_cuts(mol, cut_numbers):
    word = 0
    for k in range(3):
        word |= ((mol.bonds[cut_numbers[k]][0] | mol.bonds[cut_numbers[k]][1] << 5) if k < len(cut_numbers) else NO_CUT) << (10 * k)
    return word


def fragmentation_row(rec, n, max_nodes=DEFAULT_NODES):
    """One row of ``dsf_fraggle_fragmentations``: dict(rows [(mask, cuts, kind, sum)], summary (4), status)."""
    m = Mol(rec, n)
    if not m.usable:
        return dict(rows=[], summary=(0, 0, 0, 0), status=UNUSABLE)
    if m.fingerprint(max_nodes).over:
        return dict(rows=[], summary=(0, 0, 0, 0), status=UNDECIDED)
    chain, ring = m.cut_bonds()
    frags = m.fragmentations()
    rows = [(VM.bits(kept), pack_cuts(m, cuts), kind, total) for kind, kept, cuts, total in frags]
    return dict(rows=rows[:MAX_FRAGMENTATIONS], summary=(m.hac, len(chain), len(ring), len(rows) | (TRUNCATED if len(rows) > MAX_FRAGMENTATIONS else 0)),
                status=OK)


def fragmentation_arrays(rec, n, max_nodes=DEFAULT_NODES):
    P = len(n)
    rows, summary, status = np.full((P, MAX_FRAGMENTATIONS, 4), -1, np.int32), np.zeros((P, 4), np.int32), np.zeros(P, np.uint8)
    for p, (r, k) in enumerate(zip(np.asarray(rec), np.asarray(n))):
        row = fragmentation_row(r, k, max_nodes)
        if row["rows"]:
            rows[p, :len(row["rows"])] = np.array(row["rows"], np.int64).astype(np.int32)
        summary[p], status[p] = row["summary"], row["status"]
    return rows, summary, status


def fingerprint_arrays(rec, n, max_nodes=DEFAULT_NODES):
    """The four arrays of ``dsf_path_fingerprints``."""
    P = len(n)
    fp, atom_bits, count, status = np.zeros((P, FP_WORDS), np.int32), np.zeros((P, W, FP_WORDS), np.int32), np.zeros(P, np.int32), np.zeros(P, np.uint8)
    for p, (r, k) in enumerate(zip(np.asarray(rec), np.asarray(n))):
        m = Mol(r, k)
        if not m.usable:
            status[p] = UNUSABLE
            continue
        f = m.fingerprint(max_nodes)
        if f.over:
            status[p], count[p] = UNDECIDED, -1
            continue
        fp[p], count[p] = words(f.fp), f.count
        for a, b in f.atom_bits.items():
            atom_bits[p, a] = words(b)
    return fp, atom_bits, count, status


def better(t, best):
    """Is the Tanimoto pair ``t`` strictly above ``best`` (either = 0 counts as 1)."""
    (c1, e1), (c2, e2) = [(1, 1) if e == 0 else (c, e) for c, e in (t, best)]
    return c1 * e2 > c2 * e1


NOT_OK = dict(plain=(-1, -1), modified=(-1, -1), best_index=-1, n_fragmentations=0, marked=(0, 0), best_kind=-1, ring_step=False)


def similarity_pair(prb, ref, max_nodes=DEFAULT_NODES):
    """One row of ``dsf_fraggle_similarity_records`` for the generated record ``prb`` = (rec, n) and the ground truth ``ref``; and, beyond the
    kernel's outputs, ``best_kind`` and ``ring_step`` (the ring step of the best fragmentation marked an atom the first step did not)."""
    R, Qm = Mol(*prb), Mol(*ref)
    if not (R.usable and Qm.usable):
        return dict(NOT_OK, status=UNUSABLE)
    fq, fr = Qm.fingerprint(max_nodes), R.fingerprint(max_nodes)
    if fq.over or fr.over:
        return dict(NOT_OK, status=UNDECIDED)
    plain = (popcount(fq.fp & fr.fp), popcount(fq.fp | fr.fp))
    frags = Qm.fragmentations()
    best, best_index, best_marked, best_ring = (-1, -1), -1, (0, 0), False
    for k, (kind, kept, cuts, _) in enumerate(frags):
        A = Fingerprint(*Qm.fragment_graph(kept, cuts), max_nodes, atoms=False)
        if A.over:
            return dict(NOT_OK, status=UNDECIDED)
        (mq, first_q), (mr, first_r) = Qm.marked(A.fp, max_nodes), R.marked(A.fp, max_nodes)
        a, b = Qm.marked_fp(mq, max_nodes), R.marked_fp(mr, max_nodes)
        t = (popcount(a & b), popcount(a | b))
        if best_index < 0 or better(t, best):
            best, best_index, best_marked, best_ring = t, k, (VM.bits(mq), VM.bits(mr)), mq != first_q or mr != first_r
    return dict(plain=plain, modified=best, best_index=best_index, n_fragmentations=len(frags), marked=best_marked, status=OK,
                best_kind=frags[best_index][0] if frags else -1, ring_step=best_ring)


def similarity_table(prb_rec, prb_n, ref_rec, ref_n, ref_index=None, max_nodes=DEFAULT_NODES):
    rows = []
    for p in range(len(prb_n)):
        r = p if ref_index is None else int(ref_index[p])
        rows.append(dict(NOT_OK, status=INVALID) if not 0 <= r < len(ref_n) else similarity_pair((prb_rec[p], prb_n[p]), (ref_rec[r], ref_n[r]), max_nodes))
    return rows


KEYS = ("plain", "modified", "best_index", "n_fragmentations", "marked", "status")


def as_arrays(rows):
    """The rows of ``similarity_table`` as the six arrays of the kernel."""
    P = len(rows)
    i32 = lambda key, *shape: np.array([r[key] for r in rows], np.int64).astype(np.int32).reshape(P, *shape)
    return i32("plain", 2), i32("modified", 2), i32("best_index"), i32("n_fragmentations"), i32("marked", 2), np.array([r["status"] for r in rows], np.uint8)


def ratio(pair):
    """The float of a Tanimoto pair, as the host forms it."""
    return 1.0 if pair[1] == 0 else pair[0] / pair[1]


def fraggle(row):
    """The Fraggle similarity of a row: NaN for a pair that is not ok, 0 without a fragmentation, else the larger of plain and modified."""
    if row["status"] != OK:
        return float("nan")
    return 0.0 if row["n_fragmentations"] == 0 else max(ratio(row["plain"]), ratio(row["modified"]))


# ------------------------------------------------------------------------------------------------------------------ molecules

def _chain(k):
    return [(i, i + 1, 1) for i in range(k - 1)]


def _cycle(*atoms):
    return [(a, b, 1) for a, b in zip(atoms, atoms[1:] + atoms[:1])]


def _chain_29():
    """The 29-atom chain from the size rules: a cut i is the bond i - i+1; the left piece 0..i has size i + 2 and is kept from i = 2 on, the
    right piece i+1..28 has size 29 - i and is kept up to i = 25; 5 * sum > 3 * 29 asks for a sum of 18 at least.  With one cut a kept piece
    always is that large or the other is; with two cuts i < j the middle piece has two attachments and is dropped."""
    left, right = lambda i: list(range(i + 1)) if i >= 2 else [], lambda j: list(range(j + 1, 29)) if j <= 25 else []
    size = lambda atoms: len(atoms) + 1 if atoms else 0
    rows = [(0, left(i) + right(i), [(i, i + 1)]) for i in range(28)]
    rows += [(1, left(i) + right(j), [(i, i + 1), (j, j + 1)]) for i in range(28) for j in range(i + 1, 28) if size(left(i)) + size(right(j)) >= 18]
    return rows


def hand_table():
    """[(name, molecule, fragmentations)] with fragmentations = [(kind, kept atoms, cuts [(a, b)])] in the header's order: stated by hand from
    the header's cut bonds and size rules, not computed.  The heavy atoms come first in every molecule (G.molecule appends the hydrogens)."""
    mol, benz = G.molecule, G._ring(True)
    second_ring = [(7 + i, 7 + j, o) for i, j, o in benz]
    r6 = list(range(6))
    hexane = [
        (0, [1, 2, 3, 4, 5], [(0, 1)]), (0, [2, 3, 4, 5], [(1, 2)]), (0, [0, 1, 2, 3, 4, 5], [(2, 3)]), (0, [0, 1, 2, 3], [(3, 4)]),
        (0, [0, 1, 2, 3, 4], [(4, 5)]),
        # two cuts: the middle piece has two attachments; an end piece needs three atoms (size 4), and 5 * 4 > 3 * 6 holds
        (1, [2, 3, 4, 5], [(0, 1), (1, 2)]), (1, [3, 4, 5], [(0, 1), (2, 3)]), (1, [3, 4, 5], [(1, 2), (2, 3)]), (1, [0, 1, 2], [(2, 3), (3, 4)]),
        (1, [0, 1, 2], [(2, 3), (4, 5)]), (1, [0, 1, 2, 3], [(3, 4), (4, 5)])]
    return [
        # three atoms: no piece reaches size 4
        ("propane", mol("CCC", _chain(3), [3, 2, 3]), []),
        ("ethanol", mol("CCO", _chain(3), [3, 2, 1]), []),
        ("butane", mol("CCCC", _chain(4), [3, 2, 2, 3]), [(0, [1, 2, 3], [(0, 1)]), (0, [0, 1, 2], [(2, 3)])]),
        ("n-hexane", mol("C" * 6, _chain(6), [3, 2, 2, 2, 2, 3]), hexane),
        # the isobutyl end: atom 1 carries the methyls 0 and 5
        ("2-methylpentane", mol("C" * 6, _chain(5) + [(1, 5, 1)], [3, 1, 2, 2, 3, 3]), [
            (0, [1, 2, 3, 4, 5], [(0, 1)]), (0, [0, 1, 2, 3, 4, 5], [(1, 2)]), (0, [0, 1, 2, 3, 4], [(1, 5)]), (0, [0, 1, 2, 5], [(2, 3)]),
            (0, [0, 1, 2, 3, 5], [(3, 4)]),
            (1, [2, 3, 4], [(0, 1), (1, 2)]), (1, [2, 3, 4], [(1, 2), (1, 5)]), (1, [0, 1, 5], [(1, 2), (2, 3)]), (1, [0, 1, 5], [(1, 2), (3, 4)]),
            (1, [0, 1, 2, 5], [(2, 3), (3, 4)])]),
        # the neopentyl end: atom 1 carries the methyls 0, 5 and 6; 5 * sum > 21 asks for a sum of 5
        ("2,2-dimethylpentane", mol("C" * 7, _chain(5) + [(1, 5, 1), (1, 6, 1)], [3, 0, 2, 2, 3, 3, 3]), [
            (0, [1, 2, 3, 4, 5, 6], [(0, 1)]), (0, [0, 1, 2, 3, 4, 5, 6], [(1, 2)]), (0, [0, 1, 2, 3, 4, 6], [(1, 5)]),
            (0, [0, 1, 2, 3, 4, 5], [(1, 6)]), (0, [0, 1, 2, 5, 6], [(2, 3)]), (0, [0, 1, 2, 3, 5, 6], [(3, 4)]),
            (1, [0, 1, 5, 6], [(1, 2), (2, 3)]), (1, [0, 1, 5, 6], [(1, 2), (3, 4)]), (1, [0, 1, 2, 5, 6], [(2, 3), (3, 4)])]),
        ("toluene", mol("C" * 7, benz + [(0, 6, 1)], [0, 1, 1, 1, 1, 1, 3]), [(0, r6, [(0, 6)])]),
        ("ethylbenzene", mol("C" * 8, benz + [(0, 6, 1), (6, 7, 1)], [0, 1, 1, 1, 1, 1, 2, 3]),
         [(0, r6, [(0, 6)]), (0, r6 + [6], [(6, 7)]), (1, r6, [(0, 6), (6, 7)])]),
        # both rings are kept: the whole molecule with the bond between the rings opened
        ("biphenyl", Q._biphenyl(), [(0, list(range(12)), [(0, 6)])]),
        ("diphenylmethane", mol("C" * 13, benz + second_ring + [(0, 6, 1), (6, 7, 1)], [0, 1, 1, 1, 1, 1, 2, 0, 1, 1, 1, 1, 1]),
         [(0, list(range(13)), [(0, 6)]), (0, list(range(13)), [(6, 7)]), (1, r6 + list(range(7, 13)), [(0, 6), (6, 7)])]),
        # no chain bond and no atom with three ring bonds
        ("cyclohexane", mol("C" * 6, _cycle(0, 1, 2, 3, 4, 5), [2] * 6), []),
        ("methylcyclohexane", mol("C" * 7, _cycle(0, 1, 2, 3, 4, 5) + [(0, 6, 1)], [1, 2, 2, 2, 2, 2, 3]), [(0, r6, [(0, 6)])]),
        # fusion atoms 0 and 5: the ring with both attachments on ring atoms is kept, the opened four-atom chain is not
        ("decalin", mol("C" * 10, _cycle(0, 1, 2, 3, 4, 5) + [(0, 6, 1), (6, 7, 1), (7, 8, 1), (8, 9, 1), (9, 5, 1)], [1, 2, 2, 2, 2, 1, 2, 2, 2, 2]),
         [(2, [0, 5, 6, 7, 8, 9], [(0, 1), (4, 5)]), (2, r6, [(0, 6), (5, 9)])]),
        ("indane", mol("C" * 9, benz + [(0, 6, 1), (6, 7, 1), (7, 8, 1), (8, 5, 1)], [0, 1, 1, 1, 1, 0, 2, 2, 2]),
         [(2, [0, 5, 6, 7, 8], [(0, 1), (4, 5)]), (2, r6, [(0, 6), (5, 8)])]),
        # both attachments on the spiro atom 0
        ("spiro[4.4]nonane", mol("C" * 9, _cycle(0, 1, 2, 3, 4) + _cycle(0, 5, 6, 7, 8), [0] + [2] * 8),
         [(2, [0, 5, 6, 7, 8], [(0, 1), (0, 4)]), (2, [0, 1, 2, 3, 4], [(0, 5), (0, 8)])]),
        # kind 3: the benzene ring (two attachments on ring atoms) and the propyl chain (one); atoms 6, 7, 8 carry three attachments
        ("1-propylindane", mol("C" * 12, benz + [(0, 6, 1), (6, 7, 1), (7, 8, 1), (8, 5, 1), (6, 9, 1), (9, 10, 1), (10, 11, 1)],
                               [0, 1, 1, 1, 1, 0, 1, 2, 2, 2, 2, 3]),
         [(0, list(range(12)), [(6, 9)]), (0, list(range(10)), [(9, 10)]), (0, list(range(11)), [(10, 11)]),
          (1, list(range(9)), [(6, 9), (9, 10)]), (1, list(range(9)), [(6, 9), (10, 11)]), (1, list(range(10)), [(9, 10), (10, 11)]),
          (2, [0, 5, 6, 7, 8, 9, 10, 11], [(0, 1), (4, 5)]), (2, r6, [(0, 6), (5, 8)]),
          (3, r6 + [9, 10, 11], [(0, 6), (5, 8), (6, 9)])]),
        # bridgeheads 0 and 3 have three ring bonds: a pair of cuts frees one of the three bridges
        ("norbornane", mol("C" * 7, _cycle(0, 1, 2, 3, 4, 5) + [(0, 6, 1), (6, 3, 1)], [1, 2, 2, 1, 2, 2, 2]),
         [(2, [0, 3, 4, 5, 6], [(0, 1), (2, 3)]), (2, [0, 1, 2, 3, 6], [(0, 5), (3, 4)]), (2, r6, [(0, 6), (3, 6)])]),
        # every bond is a ring cut bond and no two cuts part the cage
        ("cubane", mol("C" * 8, _cycle(0, 1, 2, 3) + _cycle(4, 5, 6, 7) + [(0, 4, 1), (1, 5, 1), (2, 6, 1), (3, 7, 1)], [1] * 8), []),
        # hac = 8: the ethanol has no piece of size 4, and a second cut in it leaves the kept pentane piece as it is
        ("pentane and ethanol", mol("CCCCCCCO", _chain(5) + [(5, 6, 1), (6, 7, 1)], [3, 2, 2, 2, 3, 3, 2, 1]),
         [(0, [1, 2, 3, 4], [(0, 1)]), (0, [0, 1, 2, 3], [(3, 4)]), (1, [1, 2, 3, 4], [(0, 1), (5, 6)]), (1, [1, 2, 3, 4], [(0, 1), (6, 7)]),
          (1, [0, 1, 2, 3], [(3, 4), (5, 6)]), (1, [0, 1, 2, 3], [(3, 4), (6, 7)])]),
        # atom 3 is a hydrogen with two bonds: matchable, a chain atom like the others
        ("ethanol whose hydroxyl hydrogen bridges to ethyl", mol("CCOHCC", _chain(6), [3, 2, 0, 0, 2, 3]), hexane),
        ("29-atom chain", VM.chain(29), _chain_29()),
        ("naphthalene", [m for name, m, _, _ in G.hand_table() if name == "naphthalene"][0],
         [(2, [3, 4, 5, 6, 7, 8], [(2, 3), (8, 9)]), (2, [0, 1, 2, 3, 8, 9], [(3, 4), (7, 8)])]),
        ("anisole", mol("CCCCCCOC", benz + [(0, 6, 1), (6, 7, 1)], [0, 1, 1, 1, 1, 1, 0, 3]),
         [(0, r6, [(0, 6)]), (0, r6 + [6], [(6, 7)]), (1, r6, [(0, 6), (6, 7)])]),
        # the C=O bond is no cut; acetyl (three atoms, size 4) is kept beside the ring
        ("acetophenone", mol("CCCCCCCOC", benz + [(0, 6, 1), (6, 7, 2), (6, 8, 1)], [0, 1, 1, 1, 1, 1, 0, 0, 3]),
         [(0, list(range(9)), [(0, 6)]), (0, list(range(8)), [(6, 8)]), (1, r6, [(0, 6), (6, 8)])]),
    ]


def stated_rows(mol, fragmentations):
    """The hand-stated fragmentations as the (mask, cuts, kind) of ``fragmentation_row``; the cuts of a row in ascending order."""
    pack = lambda cuts: sum(((a | b << 5) if k < len(cuts) else NO_CUT) << (10 * k) for k, (a, b) in enumerate(list(cuts) + [(0, 0)] * (3 - len(cuts))))
    return [(VM.bits(kept), pack(cuts), kind) for kind, kept, cuts in fragmentations]


def moved_rows(fragmentations, perm):
    """The stated fragmentations after ``brics_mirror.renumbered(mol, perm)``, as a sorted list of (kind, kept mask, sorted cuts): the order of
    the rows within a kind moves with the numbering."""
    new = {int(old): i for i, old in enumerate(perm)}
    return sorted((kind, VM.bits(new[a] for a in kept), tuple(sorted(tuple(sorted((new[a], new[b]))) for a, b in cuts))) for kind, kept, cuts in fragmentations)


def unpacked_rows(rows):
    """Rows of ``fragmentation_row`` (or of the kernel) as the sorted list that ``moved_rows`` gives."""
    out = []
    for mask, cuts, kind, *_ in rows:
        pairs = [((cuts >> (10 * k)) & 31, (cuts >> (10 * k + 5)) & 31) for k in range(3) if (cuts >> (10 * k)) & 1023 != NO_CUT]
        out.append((int(kind), int(mask), tuple(sorted(pairs))))
    return sorted(out)


def without_atom(mol, atom):
    """``mol`` without the atom ``atom`` and without the hydrogens that hang on it alone (a deletion: its neighbour is left short of a bond)."""
    types, bond = np.asarray(mol["type"]), np.asarray(mol["bond"])
    gone = {atom} | {int(h) for h in np.nonzero(bond[atom])[0] if types[h] == H and (bond[h] > 0).sum() == 1}
    keep = [i for i in range(len(types)) if i not in gone]
    return B.renumbered(mol, np.array(keep, np.int64))


def _stripped(mol):
    """``mol`` without its plain hydrogens (they become implicit), which leaves room for substituents."""
    types, bond = np.asarray(mol["type"]), np.asarray(mol["bond"])
    keep = [i for i in range(len(types)) if not (types[i] == H and (bond[i] > 0).sum() == 1)]
    return B.renumbered(mol, np.array(keep, np.int64))


def with_heavy_atom(mol, rng):
    """``mol`` with one more F, O, N or C on an atom that has room for a single bond (a substitution of an implicit hydrogen)."""
    types, bond = [int(t) for t in mol["type"]], np.asarray(mol["bond"])
    n = len(types)
    room = [i for i in range(n) if types[i] in (1, 2) and int(bond[i].sum()) < (4 if types[i] == 1 else 3)]
    if not room or n >= W:
        return mol
    bonds = [(i, j, int(bond[i, j])) for i in range(n) for j in range(i + 1, n) if bond[i, j]]
    return VM.molecule(types + [int(rng.choice([4, 3, 2, 1]))], bonds + [(int(rng.choice(room)), n, 1)], fc=[int(c) for c in mol["fc"]] + [0])


def _bases():
    """(the table's molecules but the 29-atom chain, fused ring systems with a side chain drawn without hydrogens, small molecules without a
    fragmentation)."""
    mol = G.molecule
    table = {name: m for name, m, _ in hand_table()}
    fused = [
        mol("C" * 12, _cycle(0, 1, 2, 3, 4, 5) + [(0, 6, 1), (6, 7, 1), (7, 8, 1), (8, 9, 1), (9, 5, 1), (2, 10, 1), (10, 11, 1)], [0] * 12),     # ethyldecalin
        mol("C" * 11, _cycle(0, 1, 2, 3, 4, 5) + [(0, 6, 1), (6, 3, 1), (1, 7, 1), (7, 8, 1), (8, 9, 1), (9, 10, 1)], [0] * 11),                 # butylnorbornane
        mol("CCCCCCCCCOCC", G._ring(True) + [(0, 6, 1), (6, 7, 1), (7, 8, 1), (8, 5, 1), (2, 9, 1), (9, 10, 1), (10, 11, 1)], [0] * 12),         # ethoxyindane
        mol("C" * 13, _cycle(0, 1, 2, 3, 4) + _cycle(0, 5, 6, 7, 8) + [(2, 9, 1), (9, 10, 1), (10, 11, 1), (11, 12, 1)], [0] * 13),              # butylspirononane
        _stripped(table["1-propylindane"]),
    ]
    small = [table[name] for name in ("propane", "ethanol", "cyclohexane", "cubane")] + [
        mol("CCCCCC", G._ring(True), [1] * 6), mol("CCC", _cycle(0, 1, 2), [2] * 3), mol("COC", _chain(3), [3, 0, 3]), mol("CC", [(0, 1, 2)], [2, 2]),
        mol("CCCCC", _cycle(0, 1, 2, 3, 4), [2] * 5)]
    return [m for name, m in table.items() if name != "29-atom chain"], fused, small


def derived_pairs(seed=20261021, variants=3, fused_variants=8):
    """About 400 (generated, ground truth) pairs, fixed by the seed.  As the ground truth Q: every molecule of the table (but the 29-atom
    chain) ``variants`` times with substituents grown on (brics_mirror._grown), five fused ring systems with a side chain ``fused_variants``
    times with up to three further heavy atoms, and nine small molecules that have no fragmentation, as they are.  Against every Q three
    generated molecules - Q renumbered, Q with one more substituent (renumbered too), Q without a heavy atom that has one heavy neighbour -
    and two more substituted ones for a small Q.  Returns (prb molecules, ref molecules): pair p is prb[p] against ref[p]."""
    rng = np.random.default_rng(seed)
    plain, fused, small = _bases()
    prb, ref = [], []

    def shuffled(m):
        return B.renumbered(m, rng.permutation(len(m["type"])))

    def substituted(m):
        types, bond = np.asarray(m["type"]), np.asarray(m["bond"])
        hs = np.nonzero((types == H) & ((bond > 0).sum(1) == 1))[0]
        groups = [g for g in ("F", "OH", "NH2", "CH3") if len(types) + len(B._GROUPS[g]) - 1 <= W]
        if hs.size and groups:
            return B.substituted(m, int(rng.choice(hs)), groups[int(rng.integers(len(groups)))])
        return with_heavy_atom(m, rng)

    def deleted(m):
        types, bond = np.asarray(m["type"]), np.asarray(m["bond"])
        heavy = types != H
        ends = [i for i in np.nonzero(heavy)[0] if (bond[i][heavy] > 0).sum() == 1]
        return without_atom(m, int(rng.choice(ends))) if ends else substituted(m)

    def against(q, more=0):
        for r in [shuffled(q), shuffled(substituted(q)), deleted(q)] + [substituted(q) for _ in range(more)]:
            prb.append(r)
            ref.append(q)

    for base in plain:
        for v in range(variants):
            against(base if v == 0 else B._grown(base, rng)[0])
    for base in fused:
        for v in range(fused_variants):
            q = base
            for _ in range(v % 4):
                q = with_heavy_atom(q, rng)
            against(q)
    for base in small:
        against(base, more=2)
    return prb, ref
