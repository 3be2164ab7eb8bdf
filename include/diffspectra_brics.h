/*
 * diffspectra_brics.h - C-ABI of the BRICS analytics of libdiffspectra_hip.so: which bonds of a result record are retrosynthetic cuts, with
 * which labels, which fragment every atom falls into, and the fragments as records of their own - what the "Frag" number of the reference's
 * set metrics (evaluation/mose_metric.py:88-128, MOSES's compute_fragments / FragMetric / cos_similarity) needs per molecule, and what a
 * fragment-level analysis of a generated set is built on.  Conventions are those of diffspectra_hip.h and diffspectra_scaffold.h: plain
 * device pointers + sizes + a hipStream_t, caller-owned memory, int status (DS_OK, DS_ERR_ARG, DS_ERR_LAUNCH), stream-ordered, never
 * synchronises.
 *
 * Records.  The "single table" part of the record contract of diffspectra_hip.h, exactly as in diffspectra_substructure.h: rec [P] records of
 * DS_RECORD_BYTES bytes with the fields at the DS_REC_* offsets, 4-byte aligned; n [P] atom counts, clamped to 0..29; of an atom pair i < j the
 * bond byte at row i, column j decides (the upper triangle); bytes of atoms >= n, the lower triangle, the diagonal and the pad never
 * influence anything; P = 0 launches nothing and returns DS_OK whatever the pointers.  Atom types are 0..4 = H, C, N, O, F.
 *
 * Unusable records.  The rule of diffspectra_valence.h: n = 0, a type byte above 4 among the first n atoms, or a bond byte above 3 between two
 * atoms < n (upper triangle).  The status of such a row is DSB_UNUSABLE, its cuts and fragment_of bytes are 0xff and every other output of
 * the row is 0.
 *
 * The graph is the MATCHABLE graph of diffspectra_substructure.h: a hydrogen is FOLDED iff its charge byte is 0, it has exactly one bond, that
 * bond has order 1 and the neighbour is no hydrogen; every other atom is matchable; the bonds are those between matchable atoms.  From that
 * header and diffspectra_groups.h, unchanged: the applied charge q; aromatic atoms and aromatic bonds (two consecutive atoms of a simple cycle
 * of 5 or 6 atoms that passes the electron rule); ring bonds (the ends stay connected without the bond, judged on the graph of ALL atoms);
 * D, the number of matchable neighbours (not capped here).  In the rules below an upper-case element is a NON-AROMATIC atom of that element
 * and a lower-case element an AROMATIC one; "either case" lifts that; "chain" = not a ring bond; "single" = order 1 and not aromatic, "double"
 * = order 2 and not aromatic; "in a ring" = one of the atom's bonds is a ring bond; the neighbours that one environment names are distinct
 * atoms; every neighbour is a matchable one.
 *
 * Environments.  Restated from RDKit's BRICS.py as remembered - RDKit cannot be run where this project runs - so parity with RDKit is
 * UNPINNED; the rule is pinned by the hand-stated table of tests/brics_mirror.py.  Records hold H, C, N, O and F only, so the sulfur
 * environments L11 and L12 and the six rules that name them (4-11, 5-12, 11-13, 11-14, 11-15, 11-16) can never fire: they are left out of the
 * tables, as diffspectra_groups.h leaves sulfide and thiol unanswered.  The labels are DSB_LABELS = 1 3 4 5 6 7 8 9 10 13 14 15 16.
 *   L1   C, D = 3, with a double bond to O and another neighbour among C, N, O (either case) by any bond
 *   L3   O, D = 2, with a chain single bond to a carbon (either case) or to a matchable hydrogen
 *   L4   C, D != 1, no double bond, with a chain single bond to a carbon (either case)
 *   L5   N, D != 1, no double bond, no single bond to N, O or F (either case), and not the lactam N
 *   L6   C, not in a ring, D = 3, with a double bond to O and a chain single bond to C, N or O (either case)
 *   L7   C, D = 2 or 3, with a single bond to a carbon (either case)
 *   L8   C, not in a ring, D != 1, every bond single
 *   L9   n, q = 0, with aromatic bonds to two of {c, n, o}
 *   L10  N in a ring, with a ring bond to a C that has a double bond to O, and a ring bond to another C, N or O
 *   L13  C with a ring single bond to C, N or O and another ring single bond to N or O
 *   L14  c with an aromatic bond to c, n or o and another aromatic bond to n or o
 *   L15  C with ring single bonds to two C
 *   L16  c with aromatic bonds to two c
 * The lactam N that L5 excludes is a ring N with a ring bond to a ring C that has a double bond to O.
 *
 * Rules, in the order in which a bond takes its labels; x-y is a chain single bond between an atom of Lx and one of Ly, x=y a chain double
 * bond (DSB_NUM_RULES of them):
 *   BRICS-RULES-BEGIN
 *   1-3 1-5 1-10
 *   3-4 3-13 3-14 3-15 3-16
 *   4-5
 *   5-14 5-16 5-13 5-15
 *   6-13 6-14 6-15 6-16
 *   7=7
 *   8-9 8-10 8-13 8-14 8-15 8-16
 *   9-13 9-14 9-15 9-16
 *   10-13 10-14 10-15 10-16
 *   13-14 13-15 13-16
 *   14-14 14-15 14-16
 *   15-16
 *   16-16
 *   BRICS-RULES-END
 * A bond a-b is a CUT iff some rule (x, y) of its bond kind has a in Lx and b in Ly, or the reverse.  The first such rule in the order above
 * decides: the end that is in Lx gets label x, the other end gets y.  If both orientations fit, both ends get x.  RDKit's answer depends on
 * the atom numbering there; this is a stated deviation that keeps the result invariant under renaming atoms.  It can happen for 13-15 only:
 * it needs an atom in Lx and Ly at once, which the elements, the aromaticity or "in a ring" forbid for every other pair but 14-16, and an
 * atom of L14 and L16 has three aromatic bonds and, as a candidate of the electron rule, no fourth neighbour to be cut from.
 *
 * Invariant.  A cut is never a ring bond, and ring bonds are judged on the graph of all atoms, so every cut is a bridge of the matchable
 * graph and removing one adds exactly one component:  fragments = components of the matchable graph + cuts.
 *
 * Fragment.  A component of the matchable graph with the cuts removed, together with the folded hydrogens of its atoms.  Fragments are
 * numbered by ascending lowest atom.  A molecule without a cut is one fragment per component.
 * Attachment point.  One per cut end: it stands for the atom at the other end (RDKit's dummy [x*]) and carries the label of the atom it is
 * attached to.  The other ends of a fragment's cuts are distinct atoms outside the fragment - two bridges from one component to one atom
 * would close a cycle - so the atoms of a fragment plus its attachment points are at most n <= 29: a fragment always fits a record.
 *
 * Fragment records.  Fragment f of record p as a record of its own: its atoms in ascending original order, hydrogens included, with their
 * positions, type bytes and APPLIED charges, their bonds written symmetrically (both triangles); then its attachment points in ascending order
 * of the outside atom, each with type byte DSB_ATTACH_TYPE, charge byte = its label, the position of the outside atom and one bond, of the
 * order of the cut, to the atom it is attached to.  With aromatic = 1 every aromatic bond is written as DSB_AROMATIC_ORDER instead of its
 * Kekule order, so the two Kekule drawings of a ring give one fragment; with aromatic = 0 the Kekule orders stay.  Every other byte of the
 * row is 0.  Such records are deliberately outside the alphabet of the analytics (types 0..4, orders 0..3), which call them unusable;
 * ds_graph_hash_records and ds_graph_identity_records compare raw type, charge and bond bytes and decide fragment identity unchanged.
 *
 * Frag (computed by the caller; restates MOSES's compute_fragments, FragMetric and cos_similarity as remembered, parity unpinned).  With g_k
 * and t_k the numbers of fragments of class k among the generated and the test molecules - every occurrence counts, a molecule without a cut
 * contributes itself - Frag = sum g_k t_k / sqrt(sum g_k^2 * sum t_k^2), NaN when a side has no fragment; the three sums are exact integers.
 * Stated deviations: the rules are as remembered and unpinned against RDKit and MOSES; aromaticity is the project's rule; two fragments are
 * the same when they are the same labelled graph, not the same SMILES; there is no sanitisation filter; sulfur never occurs; the
 * both-orientations rule above.
 *
 * Method.  One wave per record, DSB_WAVES records per workgroup, an atom per lane.  The perception is that of dsq_match_records (ds_perceive.h:
 * the record scan, the fold, ring bonds by bounded reach, the aromatic cycles through the lane's own atom), which gives every lane the
 * bond-class neighbour masks of its atom.  A lane evaluates its atom's environments from those masks and a few ballots; the lower end of each
 * chain single or double bond walks the rule table; the fragments are the lowest atom reached without the cuts.  Integers only, no atomics,
 * every loop bounded by n or by the DSB_NUM_RULES rules, every output row written by its own wave: a row's outputs do not depend on the batch
 * and are bit-identical from run to run; a wave of the last workgroup without a record writes nothing.
 */
#ifndef DIFFSPECTRA_BRICS_H
#define DIFFSPECTRA_BRICS_H

#include <stdint.h>

#include "diffspectra_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DSB_OK 0
#define DSB_UNUSABLE 3
#define DSB_WAVES 4                   /* records per workgroup */
#define DSB_NUM_RULES 40
#define DSB_MAX_CUTS 28               /* bridges of a graph on 29 atoms */
#define DSB_ATTACH_TYPE 5             /* type byte of an attachment point */
#define DSB_AROMATIC_ORDER 4          /* bond byte of an aromatic bond in a fragment record */

/* Environments, cuts and fragments of every record.  Outputs, one row per record:
 *   env [P, 29] i32          bit e = the atom is in L_e (bits 1, 3..10, 13..16); 0 for a folded hydrogen and for atoms >= n
 *   cuts [P, 28, 4] u8       rows (a, b, label of a, label of b) with a < b, ascending in (a, b); unused rows are 0xff
 *   fragment_of [P, 29] u8   the fragment of every atom < n (a folded hydrogen: that of its neighbour), 0xff for atoms >= n
 *   summary [P, 4] i32       matchable atoms, cuts, fragments, atoms of the largest fragment with its hydrogens
 *   status [P] u8            DSB_OK or DSB_UNUSABLE
 * DS_ERR_ARG, checked in this order: P outside [0, 2^31 - 1]; then, for P > 0: a NULL rec, n or output; a rec that is not 4-byte aligned. */
int dsb_brics_records(const uint8_t* rec, const int32_t* n, int64_t P, int32_t* env, uint8_t* cuts, uint8_t* fragment_of, int32_t* summary,
                      uint8_t* status, void* stream);

/* The fragments as records.  first [P] i64 is the caller's exclusive prefix sum of summary[:, 2]: fragment f of record p is written to row
 * first[p] + f of the outputs; a row outside [0, F) is never written, and an unusable record has no fragment.  The analysis is computed
 * again here, not read from the outputs above (as ds_geometry_count_records / ds_geometry_fill_records split their work).  Outputs:
 *   out_rec [F] records      as "Fragment records" above
 *   out_n [F] i32            atoms plus attachment points
 *   out_owner [F] i64        the record p
 *   out_source [F, 29] u8    the original atom of every atom of the row, the outside atom for an attachment point, 0xff at and beyond out_n
 * DS_ERR_ARG, checked in this order: aromatic outside {0, 1}, F < 0, P outside [0, 2^31 - 1]; then, for P > 0: a NULL rec, n, first or
 * output; a rec or out_rec that is not 4-byte aligned.  F = 0 with P > 0 launches and writes nothing. */
int dsb_brics_fragment_records(const uint8_t* rec, const int32_t* n, int64_t P, const int64_t* first, int64_t F, int32_t aromatic,
                               uint8_t* out_rec, int32_t* out_n, int64_t* out_owner, uint8_t* out_source, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DIFFSPECTRA_BRICS_H */
