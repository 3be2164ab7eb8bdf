/*
 * diffspectra_fraggle.h - C-ABI of the Fraggle analytics of libdiffspectra_hip.so: the fragmentations of a ground-truth molecule by one, two or
 * three cuts, a branched path fingerprint with per-atom bit attribution, the "atom contribution" marking and the best Tanimoto over all
 * fragmentations - the "Fraggle similarity" line of the reference's per-pair results table (compute_metrics.py:273-291, RDKit's
 * FraggleSim.GetFraggleSimilarity(true_mol, pred_mol)).  Conventions are those of diffspectra_hip.h and diffspectra_brics.h: plain device
 * pointers + sizes + a hipStream_t, caller-owned memory, int status (DS_OK, DS_ERR_ARG, DS_ERR_LAUNCH), stream-ordered, never synchronises.
 *
 * Records.  The record contract of diffspectra_hip.h exactly as in diffspectra_substructure.h ("single table") and diffspectra_groups.h
 * ("record pairs": pair p is generated row p against ground-truth row ref_index[p], or row p when ref_index is NULL; a ref_index outside
 * [0, M) is an INVALID pair and never a read).  n is clamped to 0..29; of an atom pair i < j the bond byte at row i, column j decides; bytes
 * of atoms >= n, the lower triangle, the diagonal and the pad never influence anything; P = 0 launches nothing and returns DS_OK whatever
 * the pointers.  Unusable records: the rule of diffspectra_valence.h (n = 0, a type byte above 4 or a bond byte above 3 among atoms < n).
 *
 * RDKit cannot be run where this project runs, so the rule below is restated from RDKit's Fraggle (FraggleSim.py) and RDKFingerprint as
 * remembered, and parity with RDKit is UNPINNED; the rule is pinned by the hand-stated table of tests/fraggle_mirror.py.
 *
 * Graph.  The MATCHABLE graph of diffspectra_substructure.h: plain hydrogens are folded, applied charges are used, ring bonds are judged on
 * the graph of all atoms, aromatic atoms and bonds are the project's.  hac = the number of matchable atoms; a bond below is a bond between
 * two matchable atoms, bonds are numbered by ascending (lower atom, higher atom).
 *
 * Atom code = 2 * element + aromatic flag, with the elements H, C, N, O, F = 0..4 (a matchable hydrogen is an atom like any other) and three
 * extra codes: DSF_CODE_ATTACH (the attachment point: RDKit's dummy, atomic number 0, not aromatic), DSF_CODE_WILD (the aliphatic wildcard:
 * RDKit's Sc) and DSF_CODE_WILD_AROMATIC (RDKit's aromatic *).  Charge is not part of the code.
 * Bond class: 0 single, 1 double, 2 triple, 3 aromatic; an aromatic bond is aromatic whatever its Kekule order.
 *
 * Path fingerprint (RDKFingerprint(maxPath=5, fpSize=1024, nBitsPerHash=2, branched, with bond orders)).  Every connected set of 1..5 bonds
 * of the graph - chains, branches and cycles alike - sets 2 of DSF_FP_BITS bits, which are a function of the multiset of its bond codes and
 * the bond count k only:
 *   end code  = atom code * 8 + the degree of the atom inside the set (1..5)
 *   bond code = (the smaller end code << 9) | (the larger end code << 2) | bond class
 *   h = k;  for the codes c in ascending order:  h = mix2(h, c)       (mix2 as in diffspectra_hip.h's hash formulas: ds_rec::mix2, 64 bits)
 *   the bits are  h & 1023  and  (h >> 32) & 1023                     (they may coincide)
 * The hash is the project's own, not RDKit's: a stated deviation, like that of the Morgan fingerprint.  An atom's bits are the union of the
 * bits of the sets that have a bond at it; an atom without a bond has none.  A fingerprint is 32 words, bit b = bit b % 32 of word b / 32.
 *
 * Fragmentations of the query Q.
 *   Chain cut bond  a bond that is no ring bond, of class single ([*]!@!=!#[*]).
 *   Ring cut bond   a ring bond, of any class, with an end that has at least three ring bonds.  An order-free statement of
 *                   [R1,R2]@[r;!R1]: RDKit counts SSSR rings, which depends on the numbering in cages - a stated deviation.
 * Cutting a set of bonds gives the PIECES: the components of the matchable graph without those bonds; the other components of a
 * disconnected record are pieces with no attachment.  A piece's attachments = the cut ends in it; its SIZE = its atoms + its attachments.
 * All thresholds are integer inequalities.  Four kinds:
 *   kind 0  one chain cut;  kind 1  two chain cuts.  Kept: the pieces with exactly one attachment and size > 3.  Valid iff at least one piece
 *           is kept and 5 * (sum of the kept sizes) > 3 * hac.
 *   kind 2  two ring cuts.  There must be exactly two pieces.  A piece is valid iff both atoms that carry its attachments (they may be one
 *           atom) lie on a cycle of the piece, size > 3 and 5 * size > 2 * hac.  Every valid piece is a fragmentation of its own, the piece
 *           with the lower lowest atom first.  RDKit keeps only the later one: a stated deviation that can only raise the maximum.
 *   kind 3  a pair of ring cuts that gave at least one kind-2 fragmentation, plus one chain cut.  Pieces with three or more attachments are
 *           skipped, pieces with two are kept under the ring test of kind 2 and size > 3, pieces with one under size > 3.  Valid iff exactly
 *           two pieces are kept and 5 * (sum of the kept sizes) > 3 * hac.
 * A fragmentation is the pair (kept-atom mask, cut set).  Its FRAGMENT GRAPH: the kept atoms with their codes and their bonds without the
 * cuts, and one attachment-point atom on every cut end at a kept atom, bonded to it with the class of the cut.  Order: kind first; within a
 * kind by the cut bonds in ascending bond number (kind 3: the ring pair, then the chain cut).  No de-duplication: the result is a maximum.
 *
 * Marking (atomContrib).  A = the fingerprint of the fragment graph.  An atom of a molecule (Q or R, with its plain fingerprint) is marked iff
 * it has bits and 5 * |bits & A| < 4 * |bits| (Tversky(0, 1) < 0.8).  Then the ring step, once and not iterated: for every ring bond m-x of
 * an atom m marked in the first step, every atom v with d(m, v) + d(v, x) = d(m, x), distances in the matchable graph without that bond, is
 * marked - the atoms on the shortest ways round; the order-free stand-in for "every SSSR ring that holds a marked atom", a stated deviation.
 * A marked aromatic atom takes the code DSF_CODE_WILD_AROMATIC, any other marked atom DSF_CODE_WILD; bonds keep their class.
 *
 * Similarity.  Q = the ground truth, R = the generated record.  plain = Tanimoto(FP(Q), FP(R)); for every fragmentation f of Q,
 * T_f = Tanimoto(FP(Q marked by f), FP(R marked by f)).  A Tanimoto is the pair (common, either) = (|A & B|, |A | B|); pairs are compared by
 * cross-multiplication, either = 0 counts as 1, the lowest fragmentation index wins ties.  The caller forms fraggle = 0 when Q has no
 * fragmentation - even for identical molecules, as RDKit does - and max(plain, max_f T_f) otherwise.
 *
 * Budget.  max_nodes bounds the number of connected bond sets of one fingerprint; every set is counted exactly once, so the count is a
 * property of the graph.  A graph of more than DSF_MAX_BONDS bonds is over every budget (no record that passes the valence rule has more
 * than 58).  A row that needs a fingerprint over the budget - of the record for the first two entry points; of Q, of R or of a fragment
 * graph for the third - has the status DSF_UNDECIDED and the outputs stated below.
 *
 * Method.  One wave64 per record or pair, DSF_WAVES per workgroup, an atom per lane for the perception (ds_perceive.h, unchanged) and for the
 * pieces; the bond sets are spread over the lanes: lane e takes the sets whose lowest bond is e and grows them by adjacent higher bonds that
 * no earlier member could have added, so each set is met once.  Fingerprints and the per-atom bit rows live in LDS and are set with LDS
 * atomicOr; no global atomics, integers only, every loop bounded by n, the bond count, the budget or the fragmentation order; every output
 * row is written by its own wave: a row's outputs do not depend on the batch and are bit-identical from run to run.
 */
#ifndef DIFFSPECTRA_FRAGGLE_H
#define DIFFSPECTRA_FRAGGLE_H

#include <stdint.h>

#include "diffspectra_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DSF_OK 0
#define DSF_UNDECIDED 1
#define DSF_UNUSABLE 2
#define DSF_INVALID 3
#define DSF_WAVES 1                   /* records or pairs per workgroup: rows differ by orders of magnitude in work, so no wave waits for another */
#define DSF_MAX_NODES 1048576         /* largest budget */
#define DSF_DEFAULT_NODES 32768
#define DSF_MAX_BONDS 60
#define DSF_MAX_PATH 5
#define DSF_FP_BITS 1024
#define DSF_FP_WORDS 32
#define DSF_CODE_ATTACH 10
#define DSF_CODE_WILD 12
#define DSF_CODE_WILD_AROMATIC 13
#define DSF_NO_CUT 1023               /* an unused cut in a packed cut word */
#define DSF_MAX_FRAGMENTATIONS 256    /* rows of the listing entry point */
#define DSF_TRUNCATED 1073741824      /* bit 30 of summary[3]: the listing dropped rows */

/* The fragmentations of every record.  Outputs, one row per record:
 *   rows [P, 256, 4] i32     (kept-atom mask, cuts packed, kind, sum of the kept sizes) of the first DSF_MAX_FRAGMENTATIONS fragmentations in
 *                            the stated order; cut k in bits 10k .. 10k+9 as lower atom | higher atom << 5, DSF_NO_CUT when unused; the cuts
 *                            in the order stated above; unused rows are -1
 *   summary [P, 4] i32       hac, chain cut bonds, ring cut bonds, fragmentations (all of them) | DSF_TRUNCATED when there are more than rows
 *   status [P] u8            DSF_OK, DSF_UNDECIDED or DSF_UNUSABLE; a row that is not ok has rows = -1 and summary = 0
 * DS_ERR_ARG, checked in this order: max_nodes outside [1, DSF_MAX_NODES], P outside [0, 2^31 - 1]; then, for P > 0: a NULL rec, n or
 * output; a rec that is not 4-byte aligned. */
int dsf_fraggle_fragmentations(const uint8_t* rec, const int32_t* n, int64_t P, int32_t max_nodes, int32_t* rows, int32_t* summary, uint8_t* status,
                               void* stream);

/* The path fingerprint of every record.  Outputs, one row per record:
 *   fp [P, 32] i32           the fingerprint
 *   atom_bits [P, 29, 32] i32  the bits of every atom; 0 for a folded hydrogen and for atoms >= n
 *   count [P] i32            the number of connected bond sets; -1 for DSF_UNDECIDED, 0 for DSF_UNUSABLE
 *   status [P] u8            DSF_OK, DSF_UNDECIDED or DSF_UNUSABLE; a row that is not ok has fp = atom_bits = 0
 * DS_ERR_ARG: as above. */
int dsf_path_fingerprints(const uint8_t* rec, const int32_t* n, int64_t P, int32_t max_nodes, int32_t* fp, int32_t* atom_bits, int32_t* count,
                          uint8_t* status, void* stream);

/* The Fraggle similarity of P (generated, ground-truth) pairs; the analysis is computed here, not read from the outputs above (as
 * dsb_brics_fragment_records does).  Outputs, one row per pair:
 *   plain [P, 2] i32         (common, either) of the plain fingerprints
 *   modified [P, 2] i32      (common, either) of the best T_f; -1, -1 when Q has no fragmentation
 *   best_index [P] i32       the fragmentation that gave it, in the stated order; -1 without one
 *   n_fragmentations [P] i32 the fragmentations of Q
 *   marked [P, 2] i32        the marked-atom masks of Q and of R for the best fragmentation; 0 without one
 *   status [P] u8            DSF_OK, DSF_UNDECIDED, DSF_UNUSABLE (a record of the pair is) or DSF_INVALID (ref_index outside [0, M)), the
 *                            later winning; a pair that is not ok has plain = modified = -1, best_index = -1, n_fragmentations = 0, marked = 0
 * DS_ERR_ARG, checked in this order: max_nodes outside [1, DSF_MAX_NODES], M < 0, P outside [0, 2^31 - 1]; then, for P > 0: a NULL prb_rec,
 * prb_n or output; a prb_rec that is not 4-byte aligned; M > 0 with a NULL ref_rec or ref_n; ref_index NULL with M < P; a ref_rec that is not
 * 4-byte aligned. */
int dsf_fraggle_similarity_records(const uint8_t* prb_rec, const int32_t* prb_n, int64_t P, const uint8_t* ref_rec, const int32_t* ref_n, int64_t M,
                                   const int64_t* ref_index, int32_t max_nodes, int32_t* plain, int32_t* modified, int32_t* best_index,
                                   int32_t* n_fragmentations, int32_t* marked, uint8_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DIFFSPECTRA_FRAGGLE_H */
