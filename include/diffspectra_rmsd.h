/*
 * diffspectra_rmsd.h - C-ABI of the symmetry-corrected Kabsch RMSD of libdiffspectra_hip.so: the smallest root-mean-square distance, after the
 * best rigid fit, over ALL graph isomorphisms between a generated molecule and its ground truth - what RDKit's GetBestRMS and spyrmsd compute.
 * It is rotation invariant, bond consistent, and molecular symmetry (methyl groups, CF2, benzene, cubane) cannot inflate it; the Hungarian-
 * matched RMSD of ds_match_records (diffspectra_hip.h) is none of the three.  Conventions are those of diffspectra_hip.h: plain device
 * pointers + sizes + a hipStream_t, caller-owned memory, int status (DS_OK, DS_ERR_ARG, DS_ERR_LAUNCH), stream-ordered, never synchronises.
 *
 * Pairs, bonds, isomorphism.  Records, counts, pairing (ref_index, M) and the argument check are the "record pairs" contract of
 * diffspectra_hip.h.  A is the generated molecule (prb), B the ground truth (ref).  A bond is a bond byte > 0 (upper triangle of the record's
 * matrix).  An isomorphism phi maps the atoms of A onto the atoms of B and preserves the type byte, the charge byte and every bond byte: the
 * labels of ds_graph_identity_records.
 *
 * Selection.  atoms = DSR_ATOMS_HEAVY (0) selects the atoms whose type byte is not 0 (decoder type 0 is hydrogen, as drop_h of
 * ds_mces_records reads it); atoms = DSR_ATOMS_ALL (1) selects every atom.  An isomorphism preserves types, so the selected sets of A and B
 * correspond under every phi.  count = the number of selected atoms of A.
 *
 * Distance of one phi.  a_i and b_phi(i) are the selected positions: the record's fp32 values widened to fp64, each side centred on the
 * centroid of its own selection.  With
 *     H = sum_i a_i b_phi(i)^T,   s0 >= s1 >= s2 its singular values,   d = +1 if det H >= 0, else -1,
 *     G = sum_i |a_i|^2 + sum_i |b_i|^2   (which does not depend on phi),
 *     proper(phi)   = sqrt(max(0, (G - 2 (s0 + s1 + d s2)) / count))   the best fit by a rotation,
 *     improper(phi) = sqrt(max(0, (G - 2 (s0 + s1 - d s2)) / count))   the best fit of the mirror image of A,
 * both from one singular value decomposition.  No mass weighting.
 *
 * Outputs per pair p:
 *   verdict u8        the codes 0..3 mean what DS_GRAPH_* mean:
 *                       DSR_DIFFERENT 0  no isomorphism: proven (unequal counts, a root mismatch or an exhausted search)
 *                       DSR_DECIDED   1  the search ended and at least one phi exists: both values are minima over every phi
 *                       DSR_UNDECIDED 2  the budget max_nodes refused a try before the search could end
 *                       DSR_INVALID   3  ref_index outside [0, M): nothing is read; every output row is defined
 *   rmsd [P,2] f64    [p,0] = min over phi of proper(phi), [p,1] = min over phi of improper(phi), in the unit of the positions
 *   count i32         selected atoms of A (0 for an invalid pair), whatever the verdict
 *   nodes i32         search nodes used (0 when refinement alone decides)
 *   found i32         isomorphisms met (with twins reduced, below) until the search stopped
 *   map [P,2,29] i32  [p,0,:] and [p,1,:]: the phi that attains each minimum, as the ground-truth atom of every generated atom.  The phi with
 *                     the LARGEST s0 + s1 +- d s2 is kept, compared with "greater than": the first phi met wins a tie.  -1 in the slots >= n
 *                     and wherever no phi was tested
 * For every verdict but 1 rmsd is NaN and both maps are -1: a stopped search reports nothing it had found.
 * The values come from the trace formula above, a difference of two numbers of size G: an exact copy scores around 1e-7 A (the square root
 * of a rounding error of G / count), not 0.
 * count = 0 (HEAVY mode on H2) gives rmsd NaN (0 / 0) with verdict 1 and the first phi as both maps.  With finite positions this is the only
 * NaN rmsd of a verdict-1 pair; a position that is not finite makes the values NaN and leaves the maps -1 (no comparison with NaN holds).
 *
 * Twins.  In HEAVY mode hydrogen leaves get ordinals: two atoms of type byte 0 are twins when each has exactly one bond, to the same parent,
 * with the same bond byte and the same charge byte; an atom's ordinal is the number of its twins with a lower index, 0 for every other atom.
 * Only isomorphisms that map ordinal to ordinal are enumerated.  This loses nothing: a swap of twin hydrogens is an automorphism that fixes
 * every selected atom, every isomorphism is an ordinal-respecting one followed by such swaps, and both have the same selected images - the
 * same H, the same values.  It removes the 3! per methyl group.  Heavy leaf twins are NOT reduced: the two F of CF2 change places, and that
 * changes the heavy RMSD.  In ALL mode nothing is reduced - swapping two hydrogens changes the value - and the budget decides: neopentane has
 * 24 * 6^4 isomorphisms.
 *
 * Method: one wave64 per pair, A in lanes 0..28 and B in lanes 32..60.  A prologue loads the bonds, finds twins and ordinals, and computes
 * the centroids, G and count once.  The initial colour is the joint rank of (type, charge, ordinal); then the joint colour refinement and the
 * depth-first individualisation of ds_graph_identity_records (one SEARCH NODE per try), which goes on after every verified leaf as in
 * dsc_stereo_identity_records: every ordinal-respecting isomorphism is met exactly once.  At a leaf H is summed in one fixed order (entry by
 * entry over ascending generated atom), decomposed by the fp64 Jacobi SVD of the library's other Kabsch fits, and the two scores are
 * compared with the best so far.  Every loop is bounded (rounds <= n + 1, depth <= n, tries <= max_nodes).  No atomics: bit-identical run to
 * run and independent of the batch.
 *
 * Deviations: parity with RDKit GetBestRMS / spyrmsd is UNPINNED (neither can be run where this project runs; the definition is pinned by
 * the brute-force enumeration of tests/best_rmsd_mirror.py); no mass weighting; the ALL mode is bound by the budget.
 */
#ifndef DIFFSPECTRA_RMSD_H
#define DIFFSPECTRA_RMSD_H

#include <stdint.h>

#include "diffspectra_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DSR_DIFFERENT 0
#define DSR_DECIDED 1
#define DSR_UNDECIDED 2
#define DSR_INVALID 3
#define DSR_ATOMS_HEAVY 0
#define DSR_ATOMS_ALL 1

/* Symmetry-corrected Kabsch RMSD of (generated, ground-truth) pairs: every definition above.  max_nodes outside [0, DS_GRAPH_MAX_NODES] and
 * atoms outside {DSR_ATOMS_HEAVY, DSR_ATOMS_ALL} are DS_ERR_ARG, with the sizes, in the order of "record pairs". */
int dsr_best_rmsd_records(const uint8_t* prb_rec, const int32_t* prb_n, int64_t P, const uint8_t* ref_rec, const int32_t* ref_n, int64_t M,
                          const int64_t* ref_index, int32_t max_nodes, int32_t atoms, uint8_t* verdict, double* rmsd, int32_t* count,
                          int32_t* nodes, int32_t* found, int32_t* map, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DIFFSPECTRA_RMSD_H */
