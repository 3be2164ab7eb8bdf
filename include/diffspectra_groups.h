/*
 * diffspectra_groups.h - C-ABI of the functional-group analytics of libdiffspectra_hip.so: aromaticity perception on a result record, the 17
 * functional groups of the reference's per-pair table and their Jaccard similarity - the line "Functional Group Similarity" of
 * compute_metrics.py:273-291 (logged by run_lib.py:139-150), which the reference computes with RDKit substructure matches of the 17 patterns of
 * compute_metrics.py:38-56 and a Jaccard index of the sets of groups present (compute_metrics.py:117-144).  Conventions are those of
 * diffspectra_hip.h and diffspectra_valence.h: plain device pointers + sizes + a hipStream_t, caller-owned memory, int status (DS_OK,
 * DS_ERR_ARG, DS_ERR_LAUNCH), stream-ordered, never synchronises.
 *
 * Records.  The "single table" part of the record contract of diffspectra_hip.h: rec [P] records of DS_RECORD_BYTES bytes with the fields at
 * the DS_REC_* offsets, 4-byte aligned; n [P] atom counts, clamped to 0..29; of an atom pair i < j the bond byte at row i, column j decides
 * (the upper triangle); P = 0 launches nothing and returns DS_OK whatever the pointers.  Bytes of atoms >= n, the lower triangle, the diagonal
 * and the pad never influence anything.  Atom types are 0..4 = H, C, N, O, F.  The pair entry point follows the "record pairs" part of that
 * contract (ref_index NULL: pair p reads ground-truth row p).
 *
 * Unusable records.  The rule of diffspectra_valence.h: n = 0, a type byte above 4 among the first n atoms, or a bond byte above 3 between
 * two atoms < n (upper triangle).  Every output of an unusable row is 0 and its status is DSG_UNUSABLE.
 *
 * Per atom.
 *   q        the APPLIED charge of diffspectra_valence.h: N+1, N-1, C+1, O-1, C-1 are kept, every other charge byte counts as 0
 *   valence  the sum of the atom's bond bytes
 *   D        the number of bonded neighbours (order > 0);  Hn: the number of bonded H neighbours
 *   Vmax     the largest valence of (element, q), the table of diffspectra_valence.h: H 1; C 4, C+ 3, C- 3; N 3, N+ 4, N- 2; O 2, O- 1; F 1
 *   hi       the implicit hydrogens max(0, Vmax - valence) - what RDKit adds on sanitisation; an over-valent atom gets 0
 *   X        D + hi, the total connections;  Ht = Hn + hi, the total hydrogens
 *   dbl, trp the numbers of the atom's bonds of order 2 and of order 3
 *
 * Ring bond.  A bond a-b is a ring bond iff b can be reached from a over bonds of order > 0 without using a-b.
 *
 * Aromaticity.  This is the project's own rule, free of the bond orders' placement: the two Kekule drawings of a ring give the same atoms.
 * It restates RDKit's default model for C, N, O in rings of 5 and 6 atoms as remembered - RDKit cannot be run where this project runs - so
 * parity with RDKit is UNPINNED.  For a given cycle an atom is a CANDIDATE with an electron count e:
 *   never a candidate: H, F, any atom with trp > 0 or dbl >= 2, any atom with X > 3;
 *   C or N with dbl = 1 (C: X = 3 and q = 0; N: X = 2 and q = 0, or X = 3 and q = +1), with p the partner of the double bond:
 *        p in the cycle: e = 1;  p outside the cycle and the bond a ring bond: e = 1;
 *        p outside the cycle, the bond no ring bond and p is N or O: e = 0;  otherwise no candidate for this cycle;
 *   C with dbl = 0: X = 3 and q = -1: e = 2;  X = 3 and q = +1: e = 0;  otherwise no candidate;
 *   N with dbl = 0: X = 3 and q = 0: e = 2;  X = 2 and q = -1: e = 2;  otherwise no candidate;
 *   O: dbl = 0, X = 2 and q = 0: e = 2;  otherwise no candidate.
 * A simple cycle of 5 or of 6 atoms (over bonds of order > 0) is aromatic iff all its atoms are candidates for it and their electrons sum to
 * exactly 6; an atom is aromatic iff it lies on an aromatic cycle.  Stated deviations from RDKit: systems that are aromatic only as a fused
 * perimeter (azulene), rings of other sizes, O+ and S are not perceived.
 *
 * Groups.  Bit g of `groups` is set iff the predicate holds somewhere in the molecule - presence, not a count, as the reference keeps the
 * keys of its count dict only.  "al" = not aromatic; C#, N#, O# = the element, aromatic or not; the atoms of one match are distinct
 * (substructure matching is injective); an unspecified bond is of order 1 (a bond with an al end is a plain Kekule bond, so atom flags
 * suffice).
 *    0 alkane           al C, X = 4
 *    1 alkene           al C, X = 3, double bond to an al C with X = 3
 *    2 alkyne           al C, X = 2, triple bond to an al C
 *    3 arene            an aromatic C (the reference's second alternative, a charged aromatic carbon with X = 2, cannot arise: every candidate
 *                       carbon above has X = 3)
 *    4 alcohol          al O, X = 2, Ht = 1, single bond to a C#
 *    5 ether            al O, D = 2, both neighbours C# by single bonds
 *    6 aldehyde         al C, X = 3, Ht = 1, double bond to an al O, single bond to a C#
 *    7 ketone           al C, X = 3, double bond to an al O, single bonds to two C#
 *    8 carboxylic acid  al C, X = 3, double bond to an al O, single bond to an al O with X = 2 and Ht = 1
 *    9 ester            al C, X = 3, with a single-bonded C# r, a double bond to an al O, and a single bond to an al O that has X = 2, Ht = 0 and
 *                       a further single-bonded C# r'; r, r' and the C pairwise distinct
 *   10 haloalkane       F single-bonded to a C#
 *   11 acyl halide      al C, X = 3, double bond to an al O with X = 1, single bond to F
 *   12 amine            al N, X = 3, with no single-bonded al C neighbour that has a double bond to an al O
 *   13 amide            al N, X = 3, single bond to an al C with X = 3 that has a double bond to an al O with X = 1 and a single bond to a C#
 *   14 nitrile          al N, X = 1, triple bond to an al C with X = 2
 *   15 sulfide, 16 thiol  never set: there is no sulfur among the five types; the bits are kept so that the 17 names line up with the
 *                       reference's list
 *
 * Similarity of a pair.  With gp, gr the group words of the generated and of the ground-truth record: common = popcount(gp & gr), either =
 * popcount(gp | gr); the similarity is common / either, and 1.0 when either = 0 (compute_metrics.py:140-143) - the caller divides.  It is
 * computed for every usable pair; the reference sees only molecules that survived RDKit, and a caller who wants that filters with the valid
 * mask of dsv_valence_records.
 *
 * Method.  One wave per record or pair, DSG_WAVES per workgroup, an atom per lane; both entry points run one device routine, the pair
 * kernel on both records.  The neighbours of an atom are 29-bit masks (any order, order 1) staged per wave in LDS next to a word that holds
 * the atom's electron counts and double-bond partner.  A lane decides the ring-bond flag of its own double bond by growing the set reached
 * without it (every atom is expanded once: at most n steps), then looks for cycles with its atom as the lowest index, walking candidate
 * atoms only: they have at most three neighbours, so at most 3 * 2 * 2 * 2 * 2 partial paths per lane whatever the record.  The lanes' member
 * masks are ORed across the wave, and the predicates are per-lane tests on registers and on wave-wide masks.  Integers only, no atomics,
 * every output row written by its own wave: a row's outputs do not depend on the batch and are bit-identical from run to run.
 */
#ifndef DIFFSPECTRA_GROUPS_H
#define DIFFSPECTRA_GROUPS_H

#include <stdint.h>

#include "diffspectra_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DSG_OK 0
#define DSG_UNUSABLE 2                /* a record of the row is unusable */
#define DSG_INVALID 3                 /* ref_index outside [0, M): nothing read */
#define DSG_NUM_GROUPS 17
#define DSG_WAVES 4                   /* records or pairs per workgroup */

/* Groups and aromatic atoms of every record.  Outputs, one row per record:
 *   groups [P] i32         bit g = group g is present (bits 0..14; 15 and 16 are never set)
 *   aromatic_mask [P] i32  bit i = atom i is aromatic
 *   status [P] u8          DSG_OK or DSG_UNUSABLE (then groups and aromatic_mask are 0)
 * DS_ERR_ARG, checked in this order: P outside [0, 2^31 - 1]; then, for P > 0: a NULL rec, n or output; a rec that is not 4-byte aligned. */
int dsg_group_records(const uint8_t* rec, const int32_t* n, int64_t P, int32_t* groups, int32_t* aromatic_mask, uint8_t* status, void* stream);

/* Groups of both records of every pair and the two counts behind their Jaccard similarity.  Outputs, one row per pair:
 *   common [P] i32     popcount(gp & gr);  either [P] i32: popcount(gp | gr)
 *   groups [P, 2] i32  gp, gr: the group words of the generated and of the ground-truth record
 *   status [P] u8      DSG_OK; DSG_UNUSABLE when either record is unusable; DSG_INVALID when ref_index[p] lies outside [0, M) (neither
 *                      record is read).  A pair that is not DSG_OK has common = either = -1 and groups = 0, 0.
 * DS_ERR_ARG, checked in this order: P outside [0, 2^31 - 1] or M < 0; then, for P > 0: a NULL prb_rec, prb_n or output, a prb_rec that is not
 * 4-byte aligned; a NULL ref_rec or ref_n with M > 0; ref_index NULL with M < P; a ref_rec that is not 4-byte aligned. */
int dsg_group_similarity_records(const uint8_t* prb_rec, const int32_t* prb_n, int64_t P, const uint8_t* ref_rec, const int32_t* ref_n, int64_t M,
                                 const int64_t* ref_index, int32_t* common, int32_t* either, int32_t* groups, uint8_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DIFFSPECTRA_GROUPS_H */
