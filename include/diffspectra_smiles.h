/*
 * diffspectra_smiles.h - C-ABI of the text output of libdiffspectra_hip.so: one canonical SMILES string per result record - what the reference
 * gets from Chem.MolToSmiles (run_lib.py:111-112), mol2smiles and true_smi == pred_smi (compute_metrics.py:73-78,209-220), get_smiles and
 * set(smiles) (evaluation/mose_metric.py:12-21,103-109) - computed on the GPU and without RDKit.  Conventions are those of diffspectra_hip.h and
 * diffspectra_valence.h: plain device pointers + sizes + a hipStream_t, caller-owned memory, int status (DS_OK, DS_ERR_ARG, DS_ERR_LAUNCH),
 * stream-ordered, never synchronises.
 *
 * Records.  The "single table" part of the record contract of diffspectra_hip.h, exactly as in diffspectra_valence.h and diffspectra_scaffold.h:
 * rec [P] records of DS_RECORD_BYTES bytes with the fields at the DS_REC_* offsets, 4-byte aligned; n [P] atom counts, clamped to 0..29; of an
 * atom pair i < j the bond byte at row i, column j decides (the upper triangle); P = 0 launches nothing and returns DS_OK whatever the
 * pointers.  Bytes of atoms >= n, the lower triangle, the diagonal and the pad never influence anything; the coordinates are never read.  Atom
 * types are 0..4 = H, C, N, O, F.
 *
 * Unusable records.  n = 0, a type byte above 4 among the first n atoms, or a bond byte above 3 between two atoms < n (upper triangle).  The
 * status of such a row is DSL_UNUSABLE.
 *
 * Written graph.  A hydrogen (type 0) is FOLDED into its neighbour iff its charge byte is 0, it has exactly one bond, that bond has order 1
 * and the neighbour is not a hydrogen.  Every other atom is a written atom; its label is (type, charge byte, number of hydrogens folded into
 * it); the bonds of the written graph are the bond bytes between written atoms.  H2, a lone H, H+ and a bridging hydrogen stay written atoms.
 *
 * Canonical order.  Colours are integers; the colour of an atom is the number of written atoms that stand before its cell, so a cell's colour
 * is its first position.
 *   Initial colour   the rank of the label key (4 - type) * 65536 + charge byte * 256 + folded hydrogens: the number of written atoms with a
 *                    smaller key (F, O, N, C, H: the hetero atoms open the strings).
 *   Refinement       a round gives every written atom the signature
 *                      colour * 2^58 + ((sum over its written neighbours j of fmix(colour_j + 1) * (2 * bond byte + 1)) mod 2^64) >> 6
 *                    (fmix: the 64-bit finaliser of ds_graph_hash_records) and the new colour = the number of written atoms with a smaller
 *                    signature, compared as unsigned 64-bit numbers.  This is the total order on signatures.  The own colour leads, so a
 *                    round only splits cells; the sum is commutative, so the signature depends on the multiset of (bond byte, neighbour
 *                    colour) alone and everything commutes with renaming the atoms.  Two multisets whose sums collide share a cell that an
 *                    exact comparison would split: that costs search nodes and never the invariance.  Rounds repeat until the number of
 *                    cells stops growing (at most n + 1 rounds).
 *   Target cell      the cell of lowest colour with more than one atom.  Individualising an atom u of it: u keeps the colour, the others of
 *                    the cell get colour + 1; then the colouring is refined again.
 *   Leaf             a discrete colouring (every colour is a position).  Its certificate is the bond bytes of the written graph in canonical
 *                    positions, upper triangle, row-major.  The lexicographically smallest certificate wins; the first found wins ties.
 *   Order of tries   inside the target cell in ascending record index.  An atom u is skipped when an earlier TRIED atom v of the cell is its
 *                    twin: bond[u][k] == bond[v][k] for every written atom k other than u and v.  The transposition (u v) is then an
 *                    automorphism of the coloured graph, so the subtree below u would repeat the one below v.
 *   Budget           `nodes` counts individualisations.  Before one, if a leaf has already been reached and nodes >= max_nodes, the search
 *                    stops and the row is DSL_UNCERTIFIED: its string is a valid SMILES of the molecule (the best leaf so far), just not
 *                    the canonical one.  The first leaf always completes, so nodes can exceed max_nodes by at most n.
 *
 * Writer (an OpenSMILES subset: Kekule, no aromatic symbols, no stereo, no isotopes).
 *   Components   ordered by their lowest canonical position, joined by '.'.
 *   Walk         inside a component depth-first from the atom of lowest canonical position, neighbours in ascending canonical position; a
 *                bond to an already visited atom that is not the parent is a ring bond.
 *   Atom text    the bare symbol C N O F iff the charge is 0 and the folded hydrogen count equals the implied one: the smallest of the
 *                valences C 4, N 3 or 5, O 2, F 1 that is >= the atom's bond-order sum over written neighbours, minus that sum; 0 if no
 *                valence is large enough.  Otherwise '[' symbol, 'H' or 'Hk' (k >= 2), then '+', '-', '+k' or '-k' (k >= 2) from the signed
 *                charge byte, then ']'.  Hydrogens are always bracketed.
 *   Ring bonds   at an atom, closures to earlier visited atoms come first, in the partners' visit order, as the number only; openings come
 *                after, in the partners' visit order, as the bond symbol followed by the lowest free number.  Numbers 1..9 are a digit, 10..99
 *                are %nn.  A number released at an atom becomes free only after that atom's tokens.
 *   Children     in visit order, all but the last in parentheses, the bond symbol in front of the child: nothing for order 1, '=' for 2,
 *                '#' for 3.
 *   Overflow     more than 99 numbers open at once or more than DSL_TEXT_BYTES bytes of text is DSL_OVERFLOW (the complete graph on 29
 *                carbons is such a row).
 *
 * Stated deviations.  This is NOT RDKit's canonical form: strings of the two are compared as molecules, never as text.  The graph is the
 * constitution-level graph of ds_graph_identity_records (atom type, raw charge byte, bond order): no stereo, no isotopes, no aromaticity, no
 * normalisation of charges or tautomers.  Two Kekule drawings of one molecule give one string only where a symmetry of the molecule maps one
 * drawing onto the other (benzene: one string; 2-methylpyridine: two).  Any SMILES reader reads the strings.  Two usable records get equal
 * strings with status DSL_OK iff ds_graph_identity_records calls them identical.
 *
 * Method.  One wave per record, DSL_WAVES records per workgroup, an atom per lane.  The bond matrix (ds_rec::load_bonds) sits in LDS; folding
 * is done by ballots; the refinement is the single-molecule form of the one in ds_graph.hip (csrc/ds_refine.h holds both); the search keeps,
 * per wave in LDS, a colour byte per atom and a cell, a cursor and the tried atoms per level (depth <= n); certificates are compared with a
 * lane per row of the triangle and a ballot for the first differing row; the walk and the emission are serial in one lane (<= 29 atoms,
 * <= 406 bonds); the text is assembled in LDS and leaves as whole dwords.  Integers only, no atomics.  Every loop is bounded: rounds <= n + 1,
 * depth <= n, individualisations <= max_nodes + n, walk <= n + bonds.  A row's outputs do not depend on the batch and are bit-identical from run
 * to run; a wave of the last workgroup without a record writes nothing.
 */
#ifndef DIFFSPECTRA_SMILES_H
#define DIFFSPECTRA_SMILES_H

#include <stdint.h>

#include "diffspectra_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DSL_OK 0
#define DSL_UNCERTIFIED 1
#define DSL_OVERFLOW 2
#define DSL_UNUSABLE 3
#define DSL_TEXT_BYTES 384            /* bytes of a text row */
#define DSL_MAX_RINGS 99              /* ring numbers open at once */
#define DSL_WAVES 4                   /* records per workgroup */

/* Canonical SMILES of every record.  Outputs, one row per record, every byte of every row written:
 *   text [P, DSL_TEXT_BYTES] u8   ASCII, zero after `length`
 *   length [P] i32                bytes of text
 *   status [P] u8                 DSL_OK, DSL_UNCERTIFIED, DSL_OVERFLOW or DSL_UNUSABLE
 *   nodes [P] i32                 individualisations counted by the search (0 for an unusable row)
 *   atom_order [P, 29] i32        position of record atom i among the atoms of the string; -1 for folded hydrogens and for atoms >= n
 * For DSL_OVERFLOW and DSL_UNUSABLE `length` is 0, `text` is zero and `atom_order` is -1.
 * DS_ERR_ARG, checked in this order: max_nodes outside [0, DS_GRAPH_MAX_NODES] or P outside [0, 2^31 - 1]; then, for P > 0: a NULL rec or n; a
 * rec that is not 4-byte aligned; a NULL output; a text that is not 4-byte aligned. */
int dsl_smiles_records(const uint8_t* rec, const int32_t* n, int64_t P, int32_t max_nodes, uint8_t* text, int32_t* length, uint8_t* status,
                       int32_t* nodes, int32_t* atom_order, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DIFFSPECTRA_SMILES_H */
