/*
 * diffspectra_valence.h - C-ABI of the per-record valence analytics of libdiffspectra_hip.so: valences, 2-D / 3-D stability, validity, fragments
 * and the fragment extractor behind the reference's two first evaluation lines (run_lib.py:371-387),
 *   Metric-3D || atom stability, mol stability, validity, complete
 *   Metric-2D || atom stability, mol stability, validity, complete, unique & valid, unique & valid & novelty
 * which come from evaluation/stability.py:76-230 (check_2D_stability, get_edm_metric, get_2D_edm_metric) and evaluation/rdkit_metric.py:86-129
 * (eval_rdmol).  Conventions are those of diffspectra_hip.h: plain device pointers + sizes + a hipStream_t, caller-owned memory, int status
 * (DS_OK, DS_ERR_ARG, DS_ERR_LAUNCH), stream-ordered, never synchronises.
 *
 * Records.  Both entry points take one record table under the "single table" part of the record contract of diffspectra_hip.h: rec [P]
 * records of DS_RECORD_BYTES bytes with the fields at the DS_REC_* offsets, 4-byte aligned; n [P] atom counts, clamped to 0..29; of an atom pair
 * i < j the bond byte at row i, column j decides (the upper triangle); P = 0 launches nothing and returns DS_OK whatever the pointers.  Bytes of
 * atoms >= n, the lower triangle, the diagonal and the pad never influence anything.  Atom types are 0..4 = H, C, N, O, F.
 *
 * Bond orders (bonds_from).
 *   DSV_BONDS_RECORD    the record's bond byte of the pair; the valence of an atom is the integer sum of its bytes.
 *   DSV_BONDS_DISTANCE  the orders are decided from the record's fp32 positions by the reference's get_bond_order (evaluation/bond_analyze.py),
 *                       with exactly the arithmetic and the tables of ds_check_stability: with dx, dy, dz the fp32 differences of the
 *                       coordinates, d = fmul_rn(fsqrt_rn(fadd_rn(fadd_rn(dx dx, dy dy), dz dz)), 100) (every product rounded on its own, no
 *                       fused multiply-add); with L1, L2, L3 the single / double / triple lengths of the two elements in pm (0 = no such
 *                       bond): order 1 if d < L1 + 10, then 2 if L2 != 0 and d < L2 + 5, then 3 if L3 != 0 and d < L3 + 3, else 0.  The
 *                       record's bond and charge bytes are ignored in this mode: every charge counts as 0, also in what
 *                       dsv_fragment_records writes.
 *
 * Unusable records.  A record is unusable (status DSV_UNUSABLE) when n = 0, when a type byte among its first n atoms is above 4, or, with
 * DSV_BONDS_RECORD, when a bond byte between two atoms < n (upper triangle) is above 3.  Every other output of an unusable row is 0;
 * dsv_fragment_records writes out_n = 0 and an all-zero record.  Otherwise the status is DSV_OK.
 *
 * 2-D stability (stability.py:145-160).  With c the RAW charge byte (i8) of the atom, the atom is stable iff its valence is one of
 * allowed_fc_bonds[element][c]; a charge that is not a key of the element's table falls back to the entry for 0:
 *   H  { 0: 1,      +1: 0,         -1: 0 }
 *   C  { 0: 3 or 4, +1: 3,         -1: 3 }
 *   N  { 0: 2 or 3, +1: 2, 3 or 4, -1: 2 }
 *   O  { 0: 2,      +1: 3,         -1: 1 }
 *   F  { 0: 1,                     -1: 0 }
 * With DSV_BONDS_DISTANCE the table is allowed_bonds (stability.py:61-70, what ds_check_stability uses): H 1, C 4, N 3, O 2, F 1, equality.
 * The molecule is stable iff all n atoms are: the caller derives it as stable atoms == n.
 *
 * Validity (the Chem.SanitizeMol of rdkit_metric.mol2smiles).  The records hold no aromatic bonds, so of RDKit's sanitisation only the
 * valence check can fail.  check_2D_stability sets a formal charge on the RDKit atom only for the (element, charge) pairs of the data set's
 * atom_fc_num - N+1, N-1, C+1, O-1, C-1; every other charge byte is dropped.  That APPLIED charge q (0 where dropped, 0 for every atom with
 * DSV_BONDS_DISTANCE) decides the largest valence RDKit accepts, by its isoelectronic rule:
 *   H 1;  C 4, C+ 3, C- 3;  N 3, N+ 4, N- 2;  O 2, O- 1;  F 1.
 * An atom is valid iff valence <= that maximum (a lower valence is filled with implicit hydrogens and passes); the molecule is valid iff all
 * n atoms are.  This restates RDKit 2023.03 as remembered - RDKit cannot be run where this project runs - so parity with RDKit is UNPINNED.
 *
 * Fragments.  Connected components over ALL n atoms, hydrogens and isolated atoms included, joined by bonds of order > 0.  The largest
 * fragment is the component with most atoms; among equally large ones the one holding the lowest atom index wins (the rule of
 * ds_match_records).  A molecule is complete iff it is valid and has one fragment.
 *
 * Method.  One wave per record, DSV_WAVES records per workgroup, an atom per lane: the adjacency of an atom is a 29-bit mask in a register,
 * the components grow by ORing the masks of the atoms already reached (the reach doubles per round, so at most 5 rounds for any numbering of
 * a 29-atom chain; every loop is bounded by n).  Integers only but for the distances, no atomics, every output row written by its own
 * wave: a row's outputs do not depend on the batch and are bit-identical from run to run.
 */
#ifndef DIFFSPECTRA_VALENCE_H
#define DIFFSPECTRA_VALENCE_H

#include <stdint.h>

#include "diffspectra_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DSV_BONDS_RECORD 0
#define DSV_BONDS_DISTANCE 1
#define DSV_OK 0
#define DSV_UNUSABLE 3
#define DSV_WAVES 4                   /* records per workgroup */

/* Valences, stability, validity and fragments of every record.  Outputs, one row per record:
 *   valence [P, 29] u8      the valence of every atom < n, 0 for the others
 *   stable_mask [P] i32     bit i = atom i is stable
 *   valid_mask [P] i32      bit i = atom i is valid (the molecule is valid iff the mask is (1 << n) - 1 and the status is DSV_OK)
 *   summary [P, 4] i32      n (clamped), the number of stable atoms, the number of fragments, the atoms of the largest fragment
 *   largest_mask [P] i32    bit i = atom i belongs to the largest fragment
 *   status [P] u8           DSV_OK or DSV_UNUSABLE (then every other output of the row is 0, n included)
 * DS_ERR_ARG, checked in this order: bonds_from outside {0, 1}, P outside [0, 2^31 - 1]; then, for P > 0: a NULL rec, n or output; a rec that
 * is not 4-byte aligned. */
int dsv_valence_records(const uint8_t* rec, const int32_t* n, int64_t P, int32_t bonds_from, uint8_t* valence, int32_t* stable_mask,
                        int32_t* valid_mask, int32_t* summary, int32_t* largest_mask, uint8_t* status, void* stream);

/* The atoms of keep[p] & ((1 << n) - 1) (bit i = keep atom i) of every record as a well-formed record of their own, in ascending original
 * order: positions and types copied; the charge byte is the applied charge q above when charge_rule = 1 and the raw byte when charge_rule =
 * 0 (0 either way with DSV_BONDS_DISTANCE); the bond bytes among the kept atoms written symmetrically (with DSV_BONDS_DISTANCE the derived
 * orders); every other byte of the record 0.  out_rec [P] records, 4-byte aligned; out_n [P] i32 the number of kept atoms.  With the
 * largest_mask of dsv_valence_records this is the largest fragment of eval_rdmol; with any other mask (the heavy atoms, say) it is useful on
 * its own.  The output of a full mask is a fixed point: extracting it again with a full mask gives the same bytes.
 * DS_ERR_ARG, checked in this order: bonds_from or charge_rule outside {0, 1}, P outside [0, 2^31 - 1]; then, for P > 0: a NULL rec, n, keep,
 * out_rec or out_n; a rec or out_rec that is not 4-byte aligned. */
int dsv_fragment_records(const uint8_t* rec, const int32_t* n, int64_t P, int32_t bonds_from, const int32_t* keep, int32_t charge_rule,
                         uint8_t* out_rec, int32_t* out_n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DIFFSPECTRA_VALENCE_H */
