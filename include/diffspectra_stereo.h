/*
 * diffspectra_stereo.h - C-ABI of the stereo-aware molecular identity of libdiffspectra_hip.so: is the generated molecule the ground-truth
 * molecule as a labelled graph AND in the spatial arrangement of its four-coordinate centres and double bonds, read from the fp32 positions
 * of the result records.  The reference's "Top-1 Accuracy" compares InChIKeys (compute_metrics.py:222-230), which have a stereo layer;
 * ds_graph_identity_records (diffspectra_hip.h) is constitution-only.  Conventions are those of diffspectra_hip.h: plain device pointers +
 * sizes + a hipStream_t, caller-owned memory, int status (DS_OK, DS_ERR_ARG, DS_ERR_LAUNCH), stream-ordered, never synchronises.
 *
 * Records, counts, pairing (ref_index, M) and the argument check are the "record pairs" contract of diffspectra_hip.h.  A is the generated
 * molecule (prb), B the ground truth (ref).  A bond is a bond byte > 0 (upper triangle of the record's matrix); the neighbours of an atom are
 * the atoms < n bonded to it.  Positions are the record's fp32 values widened to fp64; every geometric quantity is fp64.
 *
 * Twins.  A LEAF is an atom with exactly one bond.  Two leaves are twins when they share parent, type byte, charge byte and the bond order
 * to the parent.  Two atoms without any bond that share type byte and charge byte are twins too.  An atom's ORDINAL is its rank by atom
 * index among its twins (the number of its twins with a lower index); it is 0 for an atom without twins.  Only isomorphisms that map
 * ordinal to ordinal are considered.  This loses nothing: swapping twins is an automorphism that touches no site below (a twin is never a
 * neighbour of a site, because its twins would be neighbours of that site as well), so every isomorphism is one that respects the ordinals
 * followed by twin swaps, and both have the same effect on every site.  It removes the 3! per methyl group from the search.
 *
 * Tetrahedral site: an atom a with exactly four neighbours, no two of them twins.  With u_1..u_4 the unit vectors from a to its neighbours
 * in ascending atom index,
 *     V = (u_1 - u_4) . ((u_2 - u_4) x (u_3 - u_4))
 * (six times the signed volume of the tetrahedron of the four unit vectors: 16 / (3 sqrt 3) = 3.08 for an ideal centre, 2.73 for a carbon
 * of cubane, 0 for a flat one; V changes sign under a reflection and under an odd permutation of the neighbours).  The site is ASSIGNED when
 * the coordinates of a and of its four neighbours are finite and |V| >= min_volume (a neighbour at the place of a gives a V that is not a
 * number, which is below every threshold).  The site's sign is + when V > 0 and - otherwise.
 *
 * E/Z site: a bond a=b of order 2 where each end has one or two other neighbours (its SUBSTITUENTS), no end has another bond of order >= 2
 * (cumulenes are out) and no end's substituents are twins.  Every atom is an end of at most one E/Z site.  For a substituent s of a and a
 * substituent t of b, with e = x_b - x_a, p = (x_s - x_a) - e ((x_s - x_a) . e) / (e . e) and q alike from x_t - x_b (the bond vectors
 * projected onto the plane normal to a -> b),
 *     c(s, t) = p . q / (|p| |q|),   the pair is CIS when c > 0.
 * The site is ASSIGNED when for every pair (s, t), at most four, the coordinates of a, b, s and t are finite, |p| > 0, |q| > 0 and
 * |c| >= min_planarity, and when, on an end with two substituents, the two pairs with the same substituent of the other end have opposite cis
 * bits.  The site's cis bit is that of (lowest substituent of a, lowest substituent of b).
 *
 * What an isomorphism phi does.  phi maps the atoms of A onto the atoms of B and preserves type byte, charge byte, every bond byte and the
 * ordinals; it therefore maps sites onto sites.
 *   phi PRESERVES the tetrahedral site a when the sign of a in A equals the sign that V has at phi(a) in B with B's neighbours taken in the
 *   order phi(n_1), .., phi(n_4): B's own sign times the parity of that order (the number of inversions among the four images, mod 2) - integers
 *   only.  phi INVERTS the site when the signs are opposite.
 *   phi preserves the E/Z site a=b when cis(lowest s of a, lowest t of b) in A equals cis(phi s, phi t) in B; for an assigned site of B that
 *   is B's cis bit, flipped once for each of phi s, phi t that is not the lowest substituent of its end.
 *   phi is SAME when it preserves every site.  phi is MIRROR when A has at least one tetrahedral site, phi inverts every tetrahedral site and
 *   preserves every E/Z site.
 *
 * Verdict per pair (u8); the codes 0..3 mean what DS_GRAPH_* mean, so a Top-K reduction over "verdict == 1" works unchanged:
 *   DSC_DIFFERENT     0  no isomorphism: proven, as in ds_graph_identity_records (unequal counts, a root mismatch or an exhausted search)
 *   DSC_IDENTICAL     1  a same phi was found and verified byte by byte
 *   DSC_UNDECIDED     2  a further try would exceed max_nodes before the search could end
 *   DSC_INVALID       3  ref_index outside [0, M): nothing is read; every output row is defined (verdict 3, zeros, map -1)
 *   DSC_MIRROR        4  search exhausted, no same phi, at least one mirror phi: an enantiomer
 *   DSC_STEREOISOMER  5  search exhausted, isomorphisms exist, none same or mirror: a diastereomer or an E/Z isomer
 *   DSC_UNASSIGNED    6  an isomorphism exists, but a site of A or of B is not assigned - a property of the two molecules, not of phi; no phi
 *                        is then tested against the sites: found[1] = found[2] = 0
 * DSC_IDENTICAL wins over DSC_MIRROR: a meso compound against its mirror image is identical.
 * When does the search stop?  exhaustive = 0: at the first same phi (-> 1), or, when a site is unassigned, at the first isomorphism (-> 6);
 * otherwise it runs until nothing is left to try.  exhaustive = 1: only when nothing is left to try - every isomorphism is enumerated, also
 * for a pair with unassigned sites.  A search that is stopped by the budget is DSC_UNDECIDED whatever it had found, so the verdict of a
 * search that ends is the same for both values.
 *
 * Outputs per pair p:
 *   verdict u8      as above
 *   nodes   i32     search nodes used (0 when refinement alone decides)
 *   found [P,3] i32 isomorphisms, same, mirror - counted until the search stopped.  With exhaustive = 1 and no budget stop found[0] of a
 *                   molecule against itself is the number of automorphisms of the ordinal-labelled graph.
 *   sites [P,4] i32 tetrahedral sites of A, E/Z sites of A (bonds), unassigned sites of A, unassigned sites of B - from each record alone,
 *                   whatever the verdict (an invalid pair: zeros)
 *   map [P,29] i32  the phi behind the verdict (ground-truth atom of every generated atom): the first same phi for DSC_IDENTICAL, the first
 *                   mirror phi for DSC_MIRROR, the first isomorphism for DSC_STEREOISOMER and DSC_UNASSIGNED; -1 everywhere otherwise
 *
 * Method: one wave64 per pair, A in lanes 0..28 and B in lanes 32..60.  A prologue per side finds twins, ordinals and the site bits (fp64, a
 * site per lane); the initial colour is the joint rank of (type, charge, ordinal); then the joint colour refinement and the depth-first
 * individualisation of ds_graph_identity_records (one SEARCH NODE per try), which here goes on after a verified leaf: every ordinal-
 * respecting isomorphism is met exactly once, because every one sends the individualised atom to exactly one atom of its class.  A verified
 * leaf is tested against the site bits in integers.  Every loop is bounded (rounds <= n + 1, depth <= n, tries <= max_nodes): a malformed
 * record ends in a verdict.  Integers only after the prologue, no atomics: bit-identical run to run and independent of the batch.
 *
 * The two thresholds are DEFINITIONS, not measurements: min_volume = 0.5 is about 16 % of the ideal 3.08, min_planarity = 0.5 is 60 degrees
 * from planar.  Nobody has measured how generated molecules distribute around them; every summary built on these verdicts reports the
 * unassigned count so that a user sees the sensitivity.
 *
 * Deviations from InChIKey equality:
 *   - still no InChI normalisation of tautomers or charges (as ds_graph_identity_records; diffspectra_mobile.h has it, and diffspectra_key.h
 *     combines it with the verdicts of this header: dsi_key_identity_records);
 *   - only four-coordinate centres: no three-coordinate N (or S, P), no allene axis, no helicity / atropisomers - a 1,3-disubstituted allene
 *     has no site and is DSC_IDENTICAL against its mirror image;
 *   - site perception is by twins (a centre with two leaf-identical neighbours is no site; a centre whose equal neighbours are larger groups
 *     IS a site, and its symmetry is found by the search as an automorphism: neopentane has one site and is identical to its mirror
 *     image), not by InChI's or CIP's rules;
 *   - parity with RDKit / InChI perception from 3-D is UNPINNED: neither can be run where this project runs.  The definition is pinned by
 *     the hand table of tests/stereo_mirror.py, a brute-force enumeration over all isomorphisms.
 */
#ifndef DIFFSPECTRA_STEREO_H
#define DIFFSPECTRA_STEREO_H

#include <stdint.h>

#include "diffspectra_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DSC_DIFFERENT 0
#define DSC_IDENTICAL 1
#define DSC_UNDECIDED 2
#define DSC_INVALID 3
#define DSC_MIRROR 4
#define DSC_STEREOISOMER 5
#define DSC_UNASSIGNED 6
#define DSC_MIN_VOLUME 0.5
#define DSC_MIN_PLANARITY 0.5
#define DSC_OK 0
#define DSC_UNUSABLE 3

/* the rows of dsc_stereo_sites' masks: bit i = atom i */
#define DSC_MASK_TETRA_SITE 0         /* a tetrahedral site */
#define DSC_MASK_TETRA_ASSIGNED 1     /* ... that is assigned */
#define DSC_MASK_TETRA_POSITIVE 2     /* ... with V > 0 */
#define DSC_MASK_EZ_SITE 3            /* an end of an E/Z site (both ends set) */
#define DSC_MASK_EZ_ASSIGNED 4        /* ... that is assigned (both ends set) */
#define DSC_MASK_EZ_CIS 5             /* ... whose (lowest substituent, lowest substituent) pair is cis (both ends set) */
#define DSC_MASK_TWIN 6               /* an atom with at least one twin */
#define DSC_NUM_MASKS 7

/* Stereo-aware identity of (generated, ground-truth) pairs: every definition above.  max_nodes outside [0, DS_GRAPH_MAX_NODES], a NaN or
 * negative min_volume or min_planarity and exhaustive outside {0, 1} are DS_ERR_ARG, with the sizes, in the order of "record pairs". */
int dsc_stereo_identity_records(const uint8_t* prb_rec, const int32_t* prb_n, int64_t P, const uint8_t* ref_rec, const int32_t* ref_n, int64_t M,
                                const int64_t* ref_index, int32_t max_nodes, double min_volume, double min_planarity, int32_t exhaustive,
                                uint8_t* verdict, int32_t* nodes, int32_t* found, int32_t* sites, int32_t* map, void* stream);

/* The twins and the sites of every record of one table (rec, n, P as in ds_graph_hash_records), one wave per record, the prologue of
 * dsc_stereo_identity_records on its own.  Outputs per record:
 *   masks [P,7] i32   the DSC_MASK_* rows above
 *   volume [P,29] f64 V of every tetrahedral site (assigned or not; it may be NaN or infinite for coincident or non-finite atoms), NaN for
 *                     every other atom and for the slots >= n
 *   status [P] u8     DSC_OK, or DSC_UNUSABLE (n = 0, a type byte above 4 among the first n atoms, a bond byte above 3 between two atoms
 *                     < n: the rule of diffspectra_valence.h; the masks of such a row are 0 and its volumes NaN)
 * (dsc_stereo_identity_records has no such rule: like ds_graph_identity_records it compares whatever bytes the records hold.)
 * A NaN or negative min_volume or min_planarity is DS_ERR_ARG, with the sizes. */
int dsc_stereo_sites(const uint8_t* rec, const int32_t* n, int64_t P, double min_volume, double min_planarity, int32_t* masks, double* volume,
                     uint8_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DIFFSPECTRA_STEREO_H */
