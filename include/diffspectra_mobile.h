/*
 * diffspectra_mobile.h - C-ABI of the mobile-hydrogen analytics of libdiffspectra_hip.so: which atoms of a result record share mobile hydrogens
 * (tautomers), how many protons the record carries beyond its neutral form, and the record rewritten in a NORMAL FORM that no longer depends
 * on where a mobile hydrogen sits, how a charge-separated acid / base pair is written, or which Kekule drawing was chosen.  Two records are
 * the same molecule at this level when their normal forms are the same labelled graph (ds_graph_identity_records / ds_graph_hash_records of
 * diffspectra_hip.h, which compare raw type, charge and bond bytes) - the level of the main layer of a standard InChI, which the reference's
 * "Top-1 Accuracy" (compute_metrics.py:222-230, an InChIKey comparison) is about.  Conventions are those of diffspectra_hip.h and
 * diffspectra_brics.h: plain device pointers + sizes + a hipStream_t, caller-owned memory, int status (DS_OK, DS_ERR_ARG, DS_ERR_LAUNCH),
 * stream-ordered, never synchronises.
 *
 * Records.  The "single table" part of the record contract of diffspectra_hip.h, exactly as in diffspectra_brics.h: rec [P] records of
 * DS_RECORD_BYTES bytes with the fields at the DS_REC_* offsets, 4-byte aligned; n [P] atom counts, clamped to 0..29; of an atom pair i < j the
 * bond byte at row i, column j decides (the upper triangle); bytes of atoms >= n, the lower triangle, the diagonal and the pad never
 * influence anything; P = 0 launches nothing and returns DS_OK whatever the pointers.  Atom types are 0..4 = H, C, N, O, F.
 *
 * Unusable records.  The rule of diffspectra_valence.h: n = 0, a type byte above 4 among the first n atoms, or a bond byte above 3 between two
 * atoms < n (upper triangle).  The status of such a row is DSM_UNUSABLE; see "Rows without an answer".
 *
 * The rule below restates InChI's mobile-H and (de)protonation normalisation as remembered - InChI cannot be run where this project runs - so
 * parity with InChI is UNPINNED; the rule is pinned by the hand-stated table of tests/mobile_mirror.py.  InChI's main layer never compares bond
 * orders: it compares the skeleton, the hydrogens fixed on each atom, the groups of atoms that share mobile hydrogens and a proton balance.
 *
 * 1. Hydrogen folding.  A hydrogen is FOLDED iff its charge byte is 0, it has exactly one bond, that bond has order 1 and the neighbour is no
 *    hydrogen (the fold of diffspectra_smiles.h, diffspectra_substructure.h and diffspectra_brics.h).  Every other atom is a KEPT atom.  Of a
 *    kept atom: q, the applied charge of diffspectra_valence.h; dbl and trp, its bonds of order 2 and 3 (their other ends are kept atoms);
 *    valence, the sum of its bond orders; Ht = its folded hydrogens + its implicit hydrogens max(0, Vmax(element, q) - valence), Vmax as in
 *    diffspectra_groups.h.
 *
 * 2. Charge normalisation, simultaneous and judged on the input.  An atom with q != 0 that is bonded to an atom whose q has the opposite sign
 *    is PAIRED and keeps q_res = q (N-oxide, nitro and ylide forms).  An unpaired N with q = +1 and Ht >= 1 gives one hydrogen: Ht -= 1,
 *    q_res = 0, p += 1.  An unpaired O or N with q = -1 takes one hydrogen: Ht += 1, q_res = 0, p -= 1.  Every other atom (C+, C-, an N+
 *    without a hydrogen) keeps q_res = q.  p is the record's proton balance.  From here on Ht is the normalised count.
 *
 * 3. Endpoints.  A CANDIDATE is an N or O with q_res = 0, trp = 0 and dbl <= 1.  A DONOR is a candidate with Ht >= 1 and dbl = 0, an ACCEPTOR
 *    a candidate with dbl = 1.  An INTERIOR atom is a C or N with q_res = 0, dbl = 1 and trp = 0 (an acceptor N is an interior atom too).
 *
 * 4. Shift path.  A SIMPLE path D = v0, v1, ..., v2k = A (no atom twice), k >= 1, from a donor to an acceptor, whose bonds have the orders
 *    1, 2, 1, 2, ..., beginning with 1 at the donor and ending with 2 at the acceptor, and whose atoms v1 ... v(2k-1) are interior atoms.
 *    D ~ A when such a path exists.  Simple matters: an alternating WALK round an odd ring can come back to the atom it entered the ring by and
 *    leave it by another bond, and so reach an acceptor that no simple path reaches.
 *
 * 5. Mobile groups.  The connected components of ~ with more than one atom, numbered by ascending lowest atom; at most DSM_MAX_GROUPS.  A
 *    group's mobile H is the sum of Ht over its members.  A member's fixed H is 0; every other kept atom's fixed H is its Ht.  A carbon is never
 *    an endpoint, so keto / enol forms are not merged (as in a standard InChI).
 *
 * 6. Search and budget.  An interior atom has one double bond, so a path is a sequence of EXTENSIONS: from the last atom u of the path (the
 *    donor, or an interior atom entered by its double bond) over a bond of order 1 to an interior atom v that is not on the path, and on over
 *    the double bond of v to its other end w.  If w is on the path the extension is dead.  If w is an acceptor, D ~ w.  If w is an interior
 *    atom the search goes on from w.  The search of a donor is depth first, v ascending, and ends when nothing is left to extend or when it
 *    has reached every acceptor of the record.  Every extension tried - every (u, v) above, dead or not - is one search NODE; the nodes of
 *    a record are the sum over its donors, which makes the order of the donors immaterial.  A record without a donor or without an acceptor
 *    spends none.  max_nodes lies in [1, DSM_MAX_NODES]; a record that needs more than max_nodes has status DSM_UNDECIDED.
 *
 * Rows without an answer.  For DSM_UNUSABLE and DSM_UNDECIDED every byte of fixed_h, group_of and group_h is 0xff and every other output of
 * the row, nodes included, is 0; the normal-form row is all 0 with out_n = 0 and out_source 0xff.  The answer depends on the record and on
 * max_nodes only, so it is the same in every run and in every batch.
 *
 * Normal form.  The record of the kept atoms in ascending original order with their positions and type bytes; the charge byte of a kept atom is
 * fixed H + 16 * (q_res + 1); the bond byte is 1 wherever two kept atoms are bonded by any order, in both triangles.  Then one GROUP NODE per
 * mobile group, in group order: type byte DSM_GROUP_TYPE, charge byte = the group's mobile H, position 0, and a bond byte 1 to every member.
 * Then, when p != 0, one bondless PROTON NODE: type byte DSM_PROTON_TYPE, charge byte p (two's complement), position 0.  Every other byte of the
 * row is 0.  More than 29 nodes (possible only for records of nearly 29 kept atoms, never for QM9) give DSM_OVERFLOW: out_n = 0 and a row as
 * in "Rows without an answer".  Such records are outside the alphabet of the analytics (types 0..4, orders 0..3), which call them unusable;
 * ds_graph_identity_records and ds_graph_hash_records rank the raw type and charge bytes without clamping and decide unchanged.  The charge
 * byte is one-to-one while fixed H <= 15, which holds for every atom within its valence.
 *
 * Stated deviations from a standard InChI: the rule is as remembered and unpinned; no stereo layer here (dsc_stereo_identity_records of
 * diffspectra_stereo.h has it on the graph as drawn; diffspectra_key.h combines the two: dsi_key_identity_records); no metal disconnection, no (+)/(-) charge migration beyond rule 2, no
 * ring-chain or 1,5-shift tautomerism beyond the paths of rule 4; a salt's components are compared as one record.  The groups are judged in one
 * pass on the drawing as given, where InChI iterates: moving one hydrogen along one path left the groups as they were in every molecule of the
 * test corpus in which no N or O is bonded to an N or O, but in a chain such as N(H)-N(H)-N=N(H) the shifted drawing N(H)-N=N-N(H2) has a path, from the first nitrogen,
 * that the input does not have, and the two drawings get different groups (tests/test_mobile_cpu.py counts such cases in its corpus).
 *
 * Method.  One wave per record, DSM_WAVES records per workgroup, an atom per lane.  The scan, the fold, the applied charge and Vmax are those
 * of ds_perceive.h.  Every donor lane runs the depth-first search of rule 6 on its own with an explicit stack in LDS (DSM_LEVELS levels: a
 * simple path on 29 atoms has at most 14 extensions), the groups are the components of ~ by pointer doubling over shuffles.  Integers only,
 * no atomics, every loop bounded by n, DSM_LEVELS or max_nodes, every output row written by its own wave: a row's outputs do not depend on
 * the batch and are bit-identical from run to run; a wave of the last workgroup without a record writes nothing.
 */
#ifndef DIFFSPECTRA_MOBILE_H
#define DIFFSPECTRA_MOBILE_H

#include <stdint.h>

#include "diffspectra_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DSM_OK 0
#define DSM_UNDECIDED 2
#define DSM_UNUSABLE 3
#define DSM_OVERFLOW 4
#define DSM_WAVES 4                   /* records per workgroup */
#define DSM_MAX_NODES 1048576         /* largest search budget of a record */
#define DSM_MAX_GROUPS 14             /* a group has two atoms at least */
#define DSM_LEVELS 15                 /* stack levels of a donor's search */
#define DSM_GROUP_TYPE 6              /* type byte of a group node */
#define DSM_PROTON_TYPE 7             /* type byte of the proton node */

/* The mobile-hydrogen analysis of every record.  Outputs, one row per record:
 *   fixed_h [P, 29] u8       fixed H of every kept atom (0 for a group member); 0xff for a folded hydrogen and for atoms >= n
 *   q_res [P, 29] i8         residual charge of every kept atom; 0 for a folded hydrogen and for atoms >= n
 *   group_of [P, 29] u8      the group of every member; 0xff elsewhere
 *   group_h [P, 14] u8       mobile H of every group; 0xff where unused
 *   summary [P, 4] i32       kept atoms, groups, mobile H in all, p
 *   nodes [P] i32            search nodes used
 *   status [P] u8            DSM_OK, DSM_UNUSABLE or DSM_UNDECIDED
 * DS_ERR_ARG, checked in this order: max_nodes outside [1, DSM_MAX_NODES], P outside [0, 2^31 - 1]; then, for P > 0: a NULL rec, n or
 * output; a rec that is not 4-byte aligned. */
int dsm_mobile_records(const uint8_t* rec, const int32_t* n, int64_t P, int32_t max_nodes, uint8_t* fixed_h, int8_t* q_res, uint8_t* group_of,
                       uint8_t* group_h, int32_t* summary, int32_t* nodes, uint8_t* status, void* stream);

/* The normal form of every record, row p of the outputs for record p.  The analysis is computed again here, not read from the outputs above
 * (as dsb_brics_fragment_records does).  Outputs:
 *   out_rec [P] records      as "Normal form" above
 *   out_n [P] i32            kept atoms + group nodes + proton node; 0 unless the status is DSM_OK
 *   out_source [P, 29] u8    the original atom of every kept atom of the row; 0xff for group nodes, the proton node and at and beyond out_n
 *   status [P] u8            DSM_OK, DSM_UNUSABLE, DSM_UNDECIDED or DSM_OVERFLOW
 * DS_ERR_ARG, checked in this order: max_nodes outside [1, DSM_MAX_NODES], P outside [0, 2^31 - 1]; then, for P > 0: a NULL rec, n or
 * output; a rec or out_rec that is not 4-byte aligned. */
int dsm_normal_records(const uint8_t* rec, const int32_t* n, int64_t P, int32_t max_nodes, uint8_t* out_rec, int32_t* out_n, uint8_t* out_source,
                       uint8_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DIFFSPECTRA_MOBILE_H */
