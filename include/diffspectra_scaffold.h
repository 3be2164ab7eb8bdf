/*
 * diffspectra_scaffold.h - C-ABI of the scaffold analytics of libdiffspectra_hip.so: the Bemis-Murcko scaffold atoms, the ring atoms and the ring
 * count of every result record - what the "Scaf" number of the reference's set metrics (evaluation/mose_metric.py:111-113, MOSES's
 * compute_scaffolds / ScafMetric) needs per molecule, and what Frag and ring statistics will want later.  Conventions are those of
 * diffspectra_hip.h and diffspectra_valence.h: plain device pointers + sizes + a hipStream_t, caller-owned memory, int status (DS_OK,
 * DS_ERR_ARG, DS_ERR_LAUNCH), stream-ordered, never synchronises.
 *
 * Records.  The "single table" part of the record contract of diffspectra_hip.h, exactly as in diffspectra_valence.h: rec [P] records of
 * DS_RECORD_BYTES bytes with the fields at the DS_REC_* offsets, 4-byte aligned; n [P] atom counts, clamped to 0..29; of an atom pair i < j the
 * bond byte at row i, column j decides (the upper triangle); P = 0 launches nothing and returns DS_OK whatever the pointers.  Bytes of atoms
 * >= n, the lower triangle, the diagonal and the pad never influence anything.  Atom types are 0..4 = H, C, N, O, F.
 *
 * Unusable records.  The rule of diffspectra_valence.h: n = 0, a type byte above 4 among the first n atoms, or a bond byte above 3 between
 * two atoms < n (upper triangle).  The status of such a row is DSK_UNUSABLE and every other output of the row is 0.
 *
 * Heavy graph.  The atoms of type 1..4 (C, N, O, F), joined by the bonds of order > 0 whose both ends are heavy.  Hydrogens and all their bonds
 * are removed first, whatever their degree: a hydrogen that bridges two rings links nothing.
 *
 * Core.  The 2-core of the heavy graph: what remains when heavy atoms with at most one remaining heavy neighbour are deleted until none is
 * left.  The result does not depend on the order of the deletions.  These are exactly the atoms on a cycle or on a path between two cycles:
 * rings plus linkers.
 *
 * Exocyclic atoms.  A heavy atom outside the core is exocyclic iff it has exactly one heavy neighbour, that neighbour is in the core, and the
 * bond to it has order >= 2 (the =O of cyclohexanone, the =O on a linker carbon).
 *
 * Scaffold = core + exocyclic atoms.  This restates RDKit's MurckoScaffold.GetScaffoldForMol as remembered - RDKit cannot be run where this
 * project runs - so parity with RDKit is UNPINNED; the rule is pinned by the hand-stated table of tests/scaffold_mirror.py.
 *
 * Ring bond, ring atom.  A core bond a-b is a ring bond iff b can be reached from a over core bonds without using a-b (the definition of
 * diffspectra_groups.h).  A core atom is a ring atom iff at least one of its core bonds is a ring bond; every other core atom is a linker
 * atom.  The linker atoms are scaffold_mask minus the ring atoms minus the exocyclic atoms, and the exocyclic atoms are the scaffold atoms
 * outside the core, so there is no output of their own.
 *
 * Rings.  The ring count is the cyclomatic number of the core: core bonds - core atoms + connected components of the core.  For a molecule
 * this is RDKit's RingInfo.NumRings() (the SSSR count), which MOSES's compute_scaffold compares with min_rings.  Exocyclic atoms do not
 * change it.
 *
 * Scaf (computed by the caller from these outputs; restates MOSES's compute_scaffolds, ScafMetric and cos_similarity as remembered, parity
 * unpinned).  A molecule has a scaffold iff its scaffold is non-empty and rings >= min_rings (MOSES's default: 2).  With g_k and t_k the
 * numbers of generated and of test molecules whose scaffold is scaffold k, Scaf = sum g_k t_k / sqrt(sum g_k^2 * sum t_k^2), NaN when either
 * side has no scaffold; the three sums are exact integers and the value is dot / sqrt(gg * tt), evaluated once on the host.
 * Stated deviations: scaffolds are identical when they are the same labelled graph (atom type, applied charge, bond order), so two Kekule
 * drawings of one scaffold are two scaffolds wherever no symmetry of the scaffold maps one drawing onto the other (2-cyclopropylpyridine:
 * N=C(R) against N-C(R)=; the two drawings of a lone benzene ring are one graph) unless the caller flattens the orders; there is no RDKit
 * sanitisation filter; a record with several fragments contributes the scaffold of all of them together.
 *
 * Method.  One wave per record, DSK_WAVES records per workgroup, an atom per lane.  The heavy neighbours of an atom are a 29-bit mask in a
 * register.  The pruning is a loop of ballots: a lane dies when popcount(neighbours & alive) <= 1; it stops when a round kills nobody and is
 * bounded by n rounds (a triangle with a 26-atom tail needs 26; the five rounds of mask doubling do not apply here).  The core neighbours are
 * staged per wave in LDS for the reach tests: a lane tests its own core bonds, growing the set reached from the far end with that one bond
 * removed until it stops growing or holds the lane's atom; every atom is expanded at most once per test, so every loop is bounded by n and
 * the complete graph on 29 atoms terminates like any other record.  The components of the core grow by the mask doubling of
 * dsv_valence_records.  Integers only, no atomics, every output row written by its own wave: a row's outputs do not depend on the batch and
 * are bit-identical from run to run; a wave of the last workgroup without a record writes nothing.
 */
#ifndef DIFFSPECTRA_SCAFFOLD_H
#define DIFFSPECTRA_SCAFFOLD_H

#include <stdint.h>

#include "diffspectra_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DSK_OK 0
#define DSK_UNUSABLE 3
#define DSK_WAVES 4                   /* records per workgroup */

/* Scaffold atoms, ring atoms and ring count of every record.  Outputs, one row per record:
 *   scaffold_mask [P] i32  bit i = atom i belongs to the scaffold (core + exocyclic atoms)
 *   ring_mask [P] i32      bit i = atom i is a ring atom (a subset of the core)
 *   summary [P, 4] i32     heavy atoms, scaffold atoms, rings, ring atoms
 *   status [P] u8          DSK_OK or DSK_UNUSABLE (then every other output of the row is 0)
 * DS_ERR_ARG, checked in this order: P outside [0, 2^31 - 1]; then, for P > 0: a NULL rec, n or output; a rec that is not 4-byte aligned. */
int dsk_scaffold_masks(const uint8_t* rec, const int32_t* n, int64_t P, int32_t* scaffold_mask, int32_t* ring_mask, int32_t* summary,
                       uint8_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DIFFSPECTRA_SCAFFOLD_H */
