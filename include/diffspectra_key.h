/*
 * diffspectra_key.h - C-ABI of the key-level molecular identity of libdiffspectra_hip.so: is the generated molecule the ground-truth molecule
 * up to mobile hydrogens, acid / base forms and Kekule drawings (the normal form of diffspectra_mobile.h) AND in the spatial arrangement of
 * its centres and double bonds (the verdicts of diffspectra_stereo.h), both at once.  The reference's "Top-1 Accuracy" compares InChIKeys
 * (compute_metrics.py:222-230); an InChIKey has a main layer, which diffspectra_mobile.h restates, and a stereo layer, which
 * diffspectra_stereo.h restates on the graph as drawn.  This header defines what a stereo site is at the normalised level, so that one
 * comparison has both.  Conventions are those of diffspectra_hip.h: plain device pointers + sizes + a hipStream_t, caller-owned memory, int
 * status (DS_OK, DS_ERR_ARG, DS_ERR_LAUNCH), stream-ordered, never synchronises.
 *
 * All of it RESTATES InChI's behaviour as remembered and is UNPINNED against InChI, which cannot be run where this project runs.  Every
 * number built on these verdicts - the key-level Top-1 above all - carries that caveat.  The definition is pinned by the hand-stated table
 * of tests/key_mirror.py.
 *
 * Graph.  The normal form of dsm_normal_records: the kept atoms in ascending original order, one group node per mobile group, the proton
 * node, every bond byte 1.  Every dsm_* definition holds unchanged (fold, charge rule, endpoints, shift paths, groups).  Every index below
 * is a NORMAL-FORM index unless it says otherwise; among kept atoms the normal-form order is the original order.
 *
 * Twins and ordinals.  As in diffspectra_stereo.h, taken on the normal form: a LEAF is a node with exactly one bond (a bond to a group node
 * counts), two leaves are twins when they share parent, type byte and charge byte (every bond byte is 1); two bondless nodes that share type
 * and charge byte are twins; the ORDINAL of a node is the number of its twins with a lower index.  The charge byte of a kept atom holds its
 * fixed hydrogens, so two methyl groups on one atom are twins, and so are two fluorines.
 *
 * Excluded atoms.  A member of a mobile group, and an atom that gave or took a proton under the charge rule (rule 2 of diffspectra_mobile.h),
 * is never a centre and never an end of an E/Z site: where its hydrogens and double bonds are drawn is what the normal form forgets.
 *
 * Hydrogen slot.  A kept atom that is not excluded, whose fixed hydrogen count is exactly 1 and that has exactly one folded hydrogen (an
 * explicit atom of the original record) has a HYDROGEN SLOT: a direction, taken from that hydrogen's position in the original record.  It
 * ranks after every kept neighbour.  Two or more fixed hydrogens are twins by analogy and give no slot; an implicit hydrogen (absent from the
 * record) gives no slot.
 *
 * Tetrahedral site: a kept atom, not excluded, whose kept neighbours plus its hydrogen slot number exactly four, no two of the neighbours
 * twins.  V, min_volume, assignment and sign are exactly those of diffspectra_stereo.h, with u_1..u_4 the unit vectors to the kept
 * neighbours in ascending index and the hydrogen slot last.
 *
 * E/Z site: a bond a-b between two kept atoms, neither excluded, for which all of this holds:
 *   - its order is 2 in the ORIGINAL record;
 *   - it is not a ring bond, ring membership judged as the substructure matcher does (over the bonds of any order of the original record).
 *     Stated deviation: InChI ignores double-bond stereo only in rings of fewer than 8 atoms;
 *   - it lies on NO shift path of the record (rule 4 of diffspectra_mobile.h: a simple alternating donor-to-acceptor path) - ALL such paths
 *     count, not only those the group search of rule 6 visits before it stops;
 *   - no end has another bond of order >= 2 in the original record;
 *   - each end has one or two SUBSTITUENTS: its kept neighbours other than the partner, plus its hydrogen slot;
 *   - no two substituents of an end are twins.
 * Cosines, min_planarity, assignment and the cis bit are those of diffspectra_stereo.h, with the substituents of an end in ascending index
 * and the hydrogen slot last; the cis bit is that of (lowest substituent of a, lowest substituent of b).
 * Consequences: the C=N of an imidic acid or an amidine is no site (it lies on the path from the OH or NH), and its amide form has none
 * either; the C=C of 3-hydroxyacrolein is no site; the C=N of an oxime IS a site (O-N=C ends on a carbon, and a carbon is never an
 * endpoint); the C=C of crotonic acid is a site whichever oxygen carries the hydrogen.
 *
 * Site search.  Marking the bonds on shift paths needs every path: every donor runs the depth-first search of rule 6 of
 * diffspectra_mobile.h, v ascending, WITHOUT its early stop; whenever an extension ends on an acceptor, every double bond of the path is
 * marked.  Every extension tried is one NODE; the nodes of a record are the sum over its donors (a record without a donor or without an
 * acceptor spends none).  The group search is a prefix of this one, so its budget is covered.  max_nodes lies in [1, DSM_MAX_NODES]; a record
 * that needs more has status DSM_UNDECIDED.
 *
 * Choices the rules leave open, made so that no output depends on the atom numbering beyond the stated "ascending index" conventions:
 * the two rejected-bond masks are independent (a ring double bond on a shift path is in both) and hold every original double bond between
 * kept atoms that is a ring bond / lies on a shift path, whatever else would have disqualified it; the hydrogen-slot flag is set for every
 * kept atom with a slot, site or not; the volume of an atom that is no tetrahedral site is 0.
 *
 * Isomorphisms: those of the two normal forms (type byte, charge byte, every bond byte, ordinals), each met once - the search of
 * dsc_stereo_identity_records, which goes on after a verified leaf.  A normal form has more of them than the drawing (the two oxygens of an
 * acid change places), and an isomorphism need not respect the original bond orders.  So:
 *   a phi that does not map A's sites onto B's sites - a centre to a centre with the same hydrogen-slot flag, an end to an end whose partner
 *   is the image of its partner and whose hydrogen-slot flag is the same, a node without a site to one without - is neither same nor mirror;
 *   otherwise phi PRESERVES / INVERTS a tetrahedral site and preserves an E/Z site as in diffspectra_stereo.h, in integers: the hydrogen
 *   slot maps to the hydrogen slot, so the parity is that of the images of the kept neighbours, and the cis bit is flipped once for each
 *   end whose lowest substituent is a kept atom whose image is not the lowest substituent of the image end.  SAME and MIRROR as there.
 *
 * Verdicts: the seven DSC_* codes of diffspectra_stereo.h with the same meanings and the same precedence.  DSC_IDENTICAL wins over
 * DSC_MIRROR; DSC_UNASSIGNED is a property of the two molecules (a site of A or of B is not assigned; no phi is tested then); a search that
 * the budget stops is DSC_UNDECIDED whatever it had found.  exhaustive as there.
 *
 * Stated deviations from InChIKey equality, beyond those of the two headers this one combines: the normalisation is one pass (deviation of
 * diffspectra_mobile.h): a shifted drawing can have other paths, hence other excluded atoms and other sites - tests/test_key_identity_cpu.py
 * counts such cases in its corpus; no keto / enol; four-coordinate centres only; ring double bonds never sites; perception by twins.
 */
#ifndef DIFFSPECTRA_KEY_H
#define DIFFSPECTRA_KEY_H

#include <stdint.h>

#include "diffspectra_hip.h"
#include "diffspectra_mobile.h"
#include "diffspectra_stereo.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the flags byte of a site row */
#define DSI_KIND_MASK 3               /* bits 0..1: DSI_KIND_* */
#define DSI_KIND_NONE 0
#define DSI_KIND_CENTRE 1             /* a tetrahedral site */
#define DSI_KIND_END 2                /* an end of an E/Z site */
#define DSI_FLAG_ASSIGNED 4           /* the site is assigned (both ends of an E/Z site) */
#define DSI_FLAG_SIGN 8               /* V > 0 of an assigned centre; the cis bit of an assigned E/Z site (both ends) */
#define DSI_FLAG_HSLOT 16             /* the atom has a hydrogen slot */
#define DSI_NO_PARTNER 255            /* partner byte of everything that is no end of an E/Z site */
#define DSI_SITE_BYTES 58             /* a site row: 29 x (flags, partner) */

/* the rows of dsi_key_sites' masks: bit i = normal-form atom i; rows 0..6 are the DSC_MASK_* rows */
#define DSI_MASK_MOBILE_BOND 7        /* an end of an original double bond between kept atoms that lies on a shift path */
#define DSI_MASK_RING_BOND 8          /* an end of an original double bond between kept atoms that is a ring bond */
#define DSI_NUM_MASKS 9

/* The sites of every record of one table (rec, n, P as in dsm_normal_records: the ORIGINAL records), one wave per record; row p lines up with
 * row p of dsm_normal_records with the same max_nodes.  Outputs per record, in normal-form numbering:
 *   site [P,29,2] u8    (flags, partner) of every node; (0, DSI_NO_PARTNER) for group nodes, the proton node and beyond
 *   masks [P,9] i32     DSC_MASK_* (twins included) and the two DSI_MASK_* rows
 *   volume [P,29] f64   V of every tetrahedral site (assigned or not; it may be NaN or infinite), 0 elsewhere
 *   nodes [P] i32       nodes of the site search
 *   status [P] u8       DSM_OK, DSM_UNDECIDED (the site search needs more than max_nodes), DSM_UNUSABLE, DSM_OVERFLOW (a normal form of more
 *                       than 29 nodes)
 * A row whose status is not DSM_OK is defined: flags 0, partner DSI_NO_PARTNER, masks 0, volumes 0, nodes 0.
 * DS_ERR_ARG, checked in this order: max_nodes outside [1, DSM_MAX_NODES], a NaN or negative min_volume or min_planarity, P outside
 * [0, 2^31 - 1]; then, for P > 0: a NULL rec, n or output; a rec that is not 4-byte aligned. */
int dsi_key_sites(const uint8_t* rec, const int32_t* n, int64_t P, int32_t max_nodes, double min_volume, double min_planarity, uint8_t* site,
                  int32_t* masks, double* volume, int32_t* nodes, uint8_t* status, void* stream);

/* Key-level identity of (generated, ground-truth) pairs: the "record pairs" contract of diffspectra_hip.h on the NORMAL-FORM records of both
 * sides (out_rec, out_n of dsm_normal_records), with the site rows of dsi_key_sites beside them: prb_site [P,29,2], ref_site [M,29,2].  A
 * row that is not DSM_OK there is an empty record here (n = 0); the caller decides what such a pair means.  Site rows are read as written by
 * dsi_key_sites; a row that contradicts its record (a centre without four slots, a partner that is no neighbour) has that site ignored.
 * Outputs verdict, nodes, found [P,3], sites [P,4], map [P,29] as dsc_stereo_identity_records; the map is in normal-form indices.
 * max_nodes outside [0, DS_GRAPH_MAX_NODES] and exhaustive outside {0, 1} are DS_ERR_ARG, with the sizes, in the order of "record pairs";
 * then, for P > 0, a NULL prb_site, and for M > 0 a NULL ref_site. */
int dsi_key_identity_records(const uint8_t* prb_rec, const int32_t* prb_n, int64_t P, const uint8_t* ref_rec, const int32_t* ref_n, int64_t M,
                             const int64_t* ref_index, const uint8_t* prb_site, const uint8_t* ref_site, int32_t max_nodes, int32_t exhaustive,
                             uint8_t* verdict, int32_t* nodes, int32_t* found, int32_t* sites, int32_t* map, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DIFFSPECTRA_KEY_H */
