"""CPU yardstick of ``dss_fold_bits`` and ``dss_tanimoto_nn`` (include/diffspectra_sets.h) in plain Python integers, on top of
``tests/morgan_mirror.py``: a bit row is ONE Python int (bit b of the row is bit b of the int), a similarity is a ``fractions.Fraction``, the sum
is ``math.fsum`` of the correctly rounded quotients.  Nothing here is shaped like the kernel: no tiles, no chunks, no words until ``words``
cuts a row up for the comparison with the device.  Also here: the set-level numbers (SNN, IntDiv, novelty) from the same pieces and
``graph_mirror.same_graph``."""
from __future__ import annotations

import math
from fractions import Fraction

from tests import graph_mirror as GM, morgan_mirror as FM


def bit_row(features, n_bits):
    """The folded feature set as one int: bit ``f mod n_bits`` set for every feature f."""
    row = 0
    for b in FM.fold(features, n_bits):
        row |= 1 << b
    return row


def words(row, n_bits):
    """The row's ``n_bits / 64`` words, unsigned: bit b of the row is bit ``b % 64`` of word ``b // 64``."""
    return [(row >> (64 * k)) & ((1 << 64) - 1) for k in range(n_bits // 64)]


def popcount(row):
    return row.bit_count() if hasattr(row, "bit_count") else bin(row).count("1")


def molecule_rows(mols, n_bits, drop_h=True, radius=2):
    """Bit rows (Python ints) of molecule dicts."""
    return [bit_row(FM.fingerprint(m, drop_h, radius), n_bits) for m in mols]


def similarity(a, b):
    """(c, u, T): T = c / u as a Fraction, 1 when both rows are empty."""
    c = popcount(a & b)
    u = popcount(a) + popcount(b) - c
    return c, u, Fraction(1) if u == 0 else Fraction(c, u)


def nearest(a_rows, b_rows, skip_same_index=False):
    """Per row of A: ``(best_common, best_union, best_index, sum, compared)``.  The nearest neighbour is the largest Fraction, among equals the
    lowest index; (-1, -1, -1) without a compared row.  ``sum`` is ``math.fsum`` of ``c / u`` as correctly rounded doubles (1.0 for u = 0)."""
    out = []
    b_sizes = [popcount(b) for b in b_rows]
    for i, a in enumerate(a_rows):
        best, terms, a_size = None, [], popcount(a)
        for j, b in enumerate(b_rows):
            if skip_same_index and j == i:
                continue
            c = popcount(a & b)
            u = a_size + b_sizes[j] - c
            t = Fraction(c, u) if u else Fraction(1)
            terms.append(1.0 if u == 0 else c / u)               # int / int in Python is the correctly rounded quotient
            if best is None or t > best[3]:
                best = (c, u, j, t)
        out.append((best[0], best[1], best[2], math.fsum(terms), len(terms)) if best else (-1, -1, -1, 0.0, 0))
    return out


def tanimoto(c, u):
    return 1.0 if u == 0 else c / u


def ordered_sum(values):
    """Doubles added one by one in index order: how the set-level numbers add up per-row results on the host.  (Not ``sum``: newer Pythons
    compensate it.)"""
    acc = 0.0
    for v in values:
        acc += v
    return acc


def ordered_mean(values):
    values = list(values)
    return ordered_sum(values) / len(values) if values else float("nan")


def snn(a_rows, b_rows):
    """Mean over the rows of A of the similarity to the nearest row of B (NaN without a row that has one)."""
    near = [tanimoto(c, u) for c, u, j, _, _ in nearest(a_rows, b_rows) if j >= 0]
    return ordered_mean(near)


def internal_diversity(rows):
    """One minus the mean similarity over all ordered pairs, self-pairs included."""
    out = nearest(rows, rows)
    pairs = sum(n for *_, n in out)
    return 1.0 - ordered_sum(s for *_, s, _ in out) / pairs if pairs else float("nan")


def classes(mols):
    """``class[p]``: the lowest row whose molecule is the same labelled graph as row p's (``graph_mirror.same_graph``)."""
    out = []
    for p, m in enumerate(mols):
        out.append(next((q for q in range(p) if out[q] == q and GM.same_graph(mols[q], m)), p))
    return out


def novelty(generated, known):
    """(novel [P] bools, distinct novel graphs / distinct generated graphs, distinct novel graphs / P)."""
    K = len(known)
    cls = classes(list(known) + list(generated))[K:]
    novel = [c >= K for c in cls]
    n_novel, n_unique = len({c for c in cls if c >= K}), len(set(cls))
    return novel, (n_novel / n_unique if cls else float("nan")), (n_novel / len(cls) if cls else float("nan"))
