/*
 * diffspectra_substructure.h - C-ABI of the substructure matcher of libdiffspectra_hip.so: does a result record contain a pattern, how many
 * times, and on which atoms.  Patterns are data (a compiled SMARTS subset, diffspectra_amd/smarts.py), so a new question is a new table row
 * and not a new kernel; the 166 MACCS keys behind the reference's "Tanimoto Similarity (MACCS)" (compute_metrics.py:248-252) are such a table
 * (diffspectra_amd/maccs.py).  That table restates RDKit's MACCSkeys.smartsPatts as remembered - RDKit cannot be run where this project
 * runs - so parity with RDKit is UNPINNED.  Conventions are those of diffspectra_groups.h: plain device pointers + sizes + a hipStream_t,
 * caller-owned memory, int status (DS_OK, DS_ERR_ARG, DS_ERR_LAUNCH), stream-ordered, never synchronises.
 *
 * Records.  The "single table" part of the record contract of diffspectra_hip.h, exactly as diffspectra_groups.h restates it (n clamped to
 * 0..29, the upper triangle decides, bytes of atoms >= n, the lower triangle, the diagonal and the pad never influence anything, P = 0
 * launches nothing and returns DS_OK whatever the pointers).  Unusable records: the rule of diffspectra_valence.h (n = 0, a type byte above 4
 * among the first n atoms, a bond byte above 3 between two atoms < n); every output of an unusable row is 0 and its status is DSQ_UNUSABLE.
 *
 * The matched graph.  A hydrogen (type 0) is FOLDED iff its charge byte is 0, it has exactly one bond, that bond has order 1 and the
 * neighbour is not a hydrogen (the "Written graph" rule of diffspectra_smiles.h).  Every other atom is a MATCHABLE atom; H2, a lone H, H+ and
 * a bridging hydrogen stay matchable, with element class H.  The bonds of the matched graph are the bonds (order > 0) between matchable atoms.
 * Atom masks in the outputs are over record atom indices; a folded hydrogen is in none of them.
 *
 * Per matchable atom (q, D, Hn, hi, X, ring bond, aromatic: the definitions of diffspectra_groups.h, on the whole record graph):
 *   element  0..4 = H, C, N, O, F;   aromatic: the atom lies on an aromatic cycle of that header's rule
 *   Ht       min(4, Hn + hi): bonded hydrogen neighbours, folded or not, plus implicit hydrogens
 *   X        min(4, number of bonded neighbours of any kind + hi)
 *   D        min(4, number of matchable neighbours)
 *   ring     1 iff one of the atom's bonds is a ring bond, else 0
 *   q        the applied charge, -1, 0 or +1
 *
 * Per bond of the matched graph: one of 8 classes, class = kind + 4 * (the bond is a ring bond), kind 0 single, 1 double, 2 triple (the
 * bond byte), 3 aromatic.  A bond is aromatic iff its two atoms are consecutive atoms of some aromatic cycle (a simple cycle of 5 or 6 atoms
 * that passes the electron rule); "both ends aromatic" does not make a bond aromatic: the bond that joins the rings of biphenyl and the
 * five-ring bond of fluorene are single.  An aromatic bond is always a ring bond, so class 3 never occurs.
 *
 * A pattern is DSQ_PATTERN_WORDS int32 words, read as unsigned:
 *   word 0            bits 0-7 the number of pattern atoms A, bits 8-15 the number of closures C
 *   word 1 + k        pattern atom k (k = 0..13), a product of allowed sets, one bit per value:
 *                       bits  0-9   element and aromaticity, bit 2 * element + aromatic
 *                       bits 10-14  Ht = 0, 1, 2, 3, >= 4        bits 15-19  X        bits 20-24  D
 *                       bits 25-26  chain atom, ring atom        bits 27-29  q = -1, 0, +1
 *                     a record atom satisfies it iff each of its six properties has its bit set; an empty set is legal and matches nothing
 *   word 15 + k       for k >= 1: bits 0-7 the parent p(k) < k, bits 8-15 the bond-class set (bit c = class c) of the bond k - p(k)
 *   word 29, 30       closure 0, 1: bits 0-7 a, bits 8-15 b, bits 16-23 the bond-class set of the bond a - b;  a < b < A
 *   every other word and bit is ignored.
 * A MALFORMED pattern - A outside 1..DSQ_MAX_PATTERN_ATOMS, C above DSQ_MAX_CLOSURES, a parent >= k, a closure without a < b < A - matches
 * nothing: count, anchors and cover are 0.  No word of a pattern is ever used as an index without these checks.
 *
 * Search.  An EMBEDDING maps the pattern atoms to distinct matchable record atoms so that every pattern atom is satisfied and the record
 * bond under every pattern bond (parent links and closures) exists and has a class of its set.  The search is defined, because truncated
 * results are part of the contract.  Every matchable record atom a that satisfies pattern atom 0 runs its own search with atom 0 on a:
 *   pattern atoms 1, 2, ... are assigned depth first; the candidates of pattern atom k are tried in ascending record index; a candidate is
 *   ASSIGNED iff it satisfies atom k, its bond to the image of p(k) has a class of the link's set, no earlier pattern atom holds it, and
 *   every closure whose later end b is k holds against the image of its a.  Every assignment (k >= 1) counts as one NODE; an assignment of
 *   the last pattern atom completes an embedding, which is recorded.  After its max_nodes-th assignment (the embedding it may have
 *   completed is recorded) a search STOPS, whether or not anything was left to try.  An entry is TRUNCATED iff one of its searches stopped;
 *   its outputs are those of the embeddings recorded.  Searches stop on their own counts, never because another one did, so the result does
 *   not depend on scheduling.  A one-atom pattern has no node.
 *
 * Method.  One wave per record, DSQ_WAVES per workgroup, an atom per lane; the prologue (properties, ring bonds by bounded mask growth,
 * aromatic cycles through the lane's own atom, the eight neighbour masks per atom in LDS) runs once per record, then the K patterns in turn:
 * one ballot per pattern atom, the per-lane stack of candidate masks in LDS (lane-interleaved), four smallest distinct atom sets per lane and
 * four rounds of "smallest above the previous" across the wave.  Integers only, no atomics, every loop bounded (a search by 2 * max_nodes + 14
 * steps), every output row written by its own wave: a row's outputs do not depend on the batch and are bit-identical from run to run.
 *
 * MACCS on top of this (diffspectra_amd/maccs.py) deviates from the reference's RDKit run in stated ways: patterns run on the
 * hydrogen-folded graph (RDKit molecules that carry hydrogens as atoms let `*` match them); aromaticity is the project's rule with the
 * deviations of diffspectra_groups.h; only applied charges count for key 49; ring keys are SMARTS cycles, as in RDKit, not SSSR rings.
 */
#ifndef DIFFSPECTRA_SUBSTRUCTURE_H
#define DIFFSPECTRA_SUBSTRUCTURE_H

#include <stdint.h>

#include "diffspectra_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DSQ_OK 0
#define DSQ_UNUSABLE 2                /* the record is unusable: every output of the row is 0 */
#define DSQ_PATTERN_WORDS 32
#define DSQ_MAX_PATTERNS 256
#define DSQ_MAX_PATTERN_ATOMS 14
#define DSQ_MAX_CLOSURES 2
#define DSQ_COUNT_CAP 4
#define DSQ_TRUNCATED 128             /* bit 7 of a count byte */
#define DSQ_MAX_NODES 16777216        /* 2^24 */
#define DSQ_DEFAULT_NODES 262144      /* 2^18: what the Python side passes when the caller names no budget */
#define DSQ_WAVES 4                   /* records per workgroup */

/* word and bit positions of a pattern */
#define DSQ_WORD_ATOM 1
#define DSQ_WORD_LINK 15
#define DSQ_WORD_CLOSURE 29
#define DSQ_BIT_ELEMENT 0
#define DSQ_BIT_HT 10
#define DSQ_BIT_X 15
#define DSQ_BIT_D 20
#define DSQ_BIT_RING 25
#define DSQ_BIT_CHARGE 27

/* Every pattern against every record.  patterns [K, 32] i32 in device memory.  Outputs, one row per record:
 *   count [P, K] u8         the number of distinct atom sets over the embeddings recorded (RDKit's uniquified match count), saturating at
 *                           DSQ_COUNT_CAP, plus DSQ_TRUNCATED when the entry is truncated
 *   anchors [P, K] i32      bit i = record atom i is the image of pattern atom 0 in a recorded embedding
 *   cover [P, K] i32        bit i = record atom i is an image in a recorded embedding
 *   aromatic_mask [P] i32   bit i = atom i is aromatic (equal to that of dsg_group_records)
 *   aromatic_rings [P] i32  the number of distinct atom sets of aromatic cycles, saturating at 4
 *   fragments [P] i32       the connected components of the matched graph (equal to those of the record graph: a folded hydrogen hangs on a
 *                           matchable atom)
 *   status [P] u8           DSQ_OK or DSQ_UNUSABLE
 * K = 0 is legal: the per-record outputs are written, patterns, count, anchors and cover may be NULL.
 * DS_ERR_ARG, checked in this order: K outside [0, DSQ_MAX_PATTERNS] or max_nodes outside [1, DSQ_MAX_NODES]; P outside [0, 2^31 - 1];
 * then, for P > 0: a NULL rec or n, a rec that is not 4-byte aligned; a NULL aromatic_mask, aromatic_rings, fragments or status; then, for
 * K > 0: a NULL patterns, count, anchors or cover; a patterns that is not 4-byte aligned. */
int dsq_match_records(const uint8_t* rec, const int32_t* n, int64_t P, const int32_t* patterns, int32_t K, int32_t max_nodes, uint8_t* count,
                      int32_t* anchors, int32_t* cover, int32_t* aromatic_mask, int32_t* aromatic_rings, int32_t* fragments, uint8_t* status,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DIFFSPECTRA_SUBSTRUCTURE_H */
