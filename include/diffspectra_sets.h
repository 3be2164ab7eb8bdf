/*
 * diffspectra_sets.h - C-ABI of the set-against-set analytics of libdiffspectra_hip.so: packed Morgan bit rows and the all-pairs Tanimoto
 * scan behind the reference's "Metric-2D" numbers SNN and IntDiv (run_lib.py:346-390, evaluation/mose_metric.py).  Conventions are those
 * of diffspectra_hip.h: plain device pointers + sizes + a hipStream_t, caller-owned memory, int status (DS_OK, DS_ERR_ARG, DS_ERR_LAUNCH),
 * stream-ordered, never synchronises.
 *
 * MOSES (the `moses` package) computes both numbers from RDKit Morgan fingerprints of radius 2 folded to 1024 bits:
 *   SNN     mean over the generated molecules of the largest Tanimoto similarity to any molecule of the test set (SNNMetric);
 *   IntDiv  1 - the mean Tanimoto similarity over all ORDERED pairs of the generated set, self-pairs included (internal_diversity, p = 1).
 * Neither MOSES nor RDKit can be run where this project runs and the reference does not vendor them: the two definitions are restated from
 * the package as remembered, and parity with MOSES is unpinned.  The fingerprints are this project's (ds_morgan_records; Kekule orders, its own
 * hash and fold), so no bit-for-bit claim against RDKit is made either.
 */
#ifndef DIFFSPECTRA_SETS_H
#define DIFFSPECTRA_SETS_H

#include <stdint.h>

#include "diffspectra_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bit rows.  A row is a fingerprint folded to n_bits, n_bits a power of two in [64, DS_MORGAN_MAX_BITS], packed into n_bits / 64 words of 64
 * bits: bit b lives in word b / 64 at position b % 64 (little-endian words, so dword b / 32, position b % 32, is the same bit).
 *
 * dss_fold_bits: (ids [P,116] u64, count [P] i32) as ds_morgan_records wrote them -> words [P, n_bits/64] u64 with bit f mod n_bits set for every
 * feature f = ids[p, k], k < count[p], and popcount [P] i32, the number of set bits of the row.  A count outside [0, 116] is clamped into that
 * range, so a malformed row cannot read outside its 116 slots.  One wave per row, the bits are ORed in LDS: no global atomics.
 * DS_ERR_ARG: P outside [0, 2^31 - 1] or a bad n_bits; then, for P > 0 (P = 0 launches nothing), a NULL pointer. */
int dss_fold_bits(const uint64_t* ids, const int32_t* count, int64_t P, int32_t n_bits, uint64_t* words, int32_t* popcount, void* stream);

/* Nearest neighbour and mean Tanimoto similarity of every row of A against all rows of B.
 * For row i of A (a_words [Na, n_bits/64], a_pop [Na] its popcounts) and every row j of B (b_words [Nb, n_bits/64], b_pop [Nb]), j != i when
 * skip_same_index = 1:
 *   c = popcount(a_i & b_j),  u = a_pop[i] + b_pop[j] - c,  T = c / u, and T = 1 when u = 0 (two empty rows: MOSES's jac[isnan] = 1).
 * a_pop and b_pop are trusted to be the rows' popcounts (dss_fold_bits writes them); they must lie in [0, n_bits].
 * Outputs, one per row of A:
 *   best_index [Na] i64   the j with the largest T.  Decided by exact integer cross-multiplication, c1 u2 > c2 u1, with u = 0 standing as
 *                         1 / 1: no floating point enters the decision.  Among equal similarities the lowest j wins.  -1: no row compared.
 *   best_common, best_union [Na] i32   c and u of that pair (0 and 0 for two empty rows); -1 and -1 when no row was compared.
 *   sum [Na] f64          the sum over the compared j of the correctly rounded quotient (double)c / (double)u, 1.0 for u = 0; 0.0 for none.
 *   compared [Na] i64     how many rows entered: Nb, or Nb - 1 when skip_same_index = 1 and i < Nb.
 * Method.  A workgroup of DSS_TILE_A lanes takes DSS_TILE_A consecutive rows of A, a row per lane with its words in registers (the kernel is
 * compiled per word count), and walks column tiles of DSS_TILE_B rows of B staged in LDS, which all lanes read at the same address (a
 * broadcast).  Per dword of a pair the work is one AND and one population count that accumulates; per pair one fp64 division.
 * Order.  The column tiles are dealt to K = min(DSS_CHUNKS, number of column tiles) chunks: chunk g takes tiles g, g + K, g + 2K, ... in
 * ascending order and visits the rows of a tile in ascending j.  A lane adds its quotients in that order in fp64 and leaves (c, u, j, sum) of
 * its chunk in the workspace; a last kernel merges the K partials of a row in chunk order (a tie between chunks goes to the lower j).  No
 * atomics on any output: the result is bit-identical from run to run, and the order of summation depends only on (Na, Nb, n_bits).
 * Limits.  c and u stay below 2^13, so the cross-multiplication is done in 32 bits.
 * workspace: caller-owned device memory, 8-byte aligned, at least dss_tanimoto_nn_workspace_bytes(Na, Nb) bytes (a pure host function; the
 * size does not decrease with Nb), private layout.
 * DS_ERR_ARG: Na or Nb outside [0, 2^31 - 1], a bad n_bits, skip_same_index outside {0, 1}; then, for Na > 0 (Na = 0 launches nothing): a
 * NULL output, a NULL a_words or a_pop, an a_words or b_words that is not 16-byte aligned (8-byte at n_bits = 64), a NULL b_words or b_pop
 * with Nb > 0, a NULL, too small or misaligned workspace with Nb > 0.  Nb = 0 writes the "no row compared" values. */
#define DSS_TILE_A 256
#define DSS_TILE_B 64
#define DSS_CHUNKS 32
int dss_tanimoto_nn_workspace_bytes(int64_t Na, int64_t Nb, int64_t* bytes);
int dss_tanimoto_nn(const uint64_t* a_words, const int32_t* a_pop, int64_t Na, const uint64_t* b_words, const int32_t* b_pop, int64_t Nb,
                    int32_t n_bits, int32_t skip_same_index, void* workspace, int64_t workspace_bytes, int32_t* best_common, int32_t* best_union,
                    int64_t* best_index, double* sum, int64_t* compared, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DIFFSPECTRA_SETS_H */
