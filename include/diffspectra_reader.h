/*
 * diffspectra_reader.h - C-ABI of the text input of libdiffspectra_hip.so: one result record per SMILES string - what the reference gets from
 * Chem.MolFromSmiles (compute_metrics.py:96-114,147-317; evaluation/rdkit_metric.py:86) - computed on the GPU and without RDKit.  It is the
 * inverse direction of diffspectra_smiles.h, and its conventions are the same: plain device pointers + sizes + a hipStream_t, caller-owned
 * memory, int status (DS_OK, DS_ERR_ARG, DS_ERR_LAUNCH), stream-ordered, never synchronises; every byte of every output row is written; P = 0
 * launches nothing and returns DS_OK whatever the pointers.
 *
 * Input.  text [P, stride] u8: one ASCII row per string, of which the first length[p] bytes are read; stride is a multiple of 4 in
 * [4, DSP_TEXT_BYTES] and text is 4-byte aligned (rows are read as dwords).  DSP_TEXT_BYTES = DSL_TEXT_BYTES, so the text / length outputs of
 * dsl_smiles_records are an input as they stand.  length[p] > stride or < 0 is DSP_TOO_LONG and the row is not read; length[p] = 0 is DSP_EMPTY.
 *
 * Accepted language (an OpenSMILES subset; everything else is an error with the offset of its first offending byte).
 *   Atoms        bare  C N O F c n o .  Bracket atoms  '[' isotope? symbol chiral? hcount? charge? class? ']'  with
 *                  isotope  one or more digits (read and ignored, flag bit 0)
 *                  symbol   H C N O F c n o
 *                  chiral   '@' or '@@' (read and ignored, flag bit 1)
 *                  hcount   'H' or 'H' and one digit
 *                  charge   '+', '-', '++', '--', or a sign and 1..3 digits of a value <= 127
 *                  class    ':' and one or more digits (read and ignored, flag bit 3)
 *                Lower case marks an atom as written aromatic (flag bit 4).  H is legal only in brackets.
 *   Elements     A well-formed atom outside H C N O F is DSP_ELEMENT, not DSP_SYNTAX: bare B S P I b s p *, bare Cl (a C followed by l) and
 *                Br, in brackets b s p *, any capital other than H C N O F, and any capital followed by a lower-case letter ([Na+], [Cl-],
 *                [Co]).  `where` is the offset of the symbol's first letter.
 *   Bonds        '-' '=' '#' ':' '/' '\'.  '/' and '\' read as '-' and set flag bit 2.  ':' reads exactly like an unwritten bond (below).
 *                A bond symbol needs an atom before it in its component and an atom or a ring number after it; two symbols in a row, a
 *                symbol before '(' ')' '.' or at the end are DSP_SYNTAX.  '$' is DSP_SYNTAX, as is every other byte not named here.
 *   Branches     '(' after an atom, a ring number or ')'; it must be followed by an atom or by a bond symbol and an atom.  '()', '((' ,
 *                '(' before the first atom of a component, a ring number or '.' directly after '(' (also behind the branch's bond symbol), ')'
 *                without an open '(' and '.' inside a branch are DSP_SYNTAX.
 *   Ring numbers one digit 0..9 or '%' and two digits; they belong to the atom before them.  The first use opens, the second closes, and
 *                the number is free again.  A bond symbol may stand in front of either use or of both; two different bonds ('/' '\' count as
 *                '-'), a closure of an atom onto itself, a second bond between two atoms that are already bonded are DSP_SYNTAX at the closing
 *                number (its digit or its '%').  '%' without two digits is DSP_SYNTAX at the '%'.
 *   Dot          '.' after an atom, a ring number or ')' outside every branch; an atom must follow.  Open ring numbers cross a dot.
 *   End of text  Left open at the end, each at the offset given, are DSP_SYNTAX: a bracket atom (its '['), a bond symbol, '(' or '.' that still
 *                waits for its atom (that byte), a branch (its '(', the outermost one), a ring number (its opening digit or '%').  Of
 *                several the lowest offset is reported.
 *   First error  The text is read from left to right and the first offending byte decides status and `where`.
 *
 * Graph.  The atoms of the string in string order; a bond from every atom to the atom before it (the last atom before the branch for the
 * first atom of a branch; none after a dot) and one per ring number.  A written '-' '/' '\' is order 1, '=' 2, '#' 3.  An unwritten bond
 * or ':' is AROMATIC iff both its atoms are lower case and it is a ring bond of the string's graph (its ends stay connected without it);
 * otherwise it is single: c1ccccc1c1ccccc1 is biphenyl, C:C is ethane.
 *
 * Size.  A string with more than 29 atoms is DSP_TOO_LARGE (where = -1) once its whole text has been read without an error; the Kekule
 * search is not run on it.
 *
 * Kekule structure.  sigma = an aromatic atom's bond-order sum with aromatic bonds counted 1; h = its bracket hydrogen count (0 for a bare
 * atom); V = C 4, C+ 3, C- 3, N 3, N+ 4, N- 2, O 2, O+ 3 and 0 for every other charge.  A lower-case atom WANTS a double bond iff
 * V - sigma - h >= 1.  The double bonds are a perfect matching of the wanting atoms along aromatic bonds, namely the first one in this
 * depth-first order: take the unmatched wanting atom u of lowest string index and try its unmatched wanting aromatic neighbours in
 * ascending string index; with u matched go on to the next u; when u has no neighbour left, undo the latest try and continue at that
 * level.  `nodes` counts tries; before a try, nodes >= max_nodes is DSP_UNDECIDED (where = -1).  When nothing is left to undo there is no
 * Kekule structure: DSP_KEKULE, and `where` is the symbol of the atom u of the LAST dead end, a dead end being a u that found no
 * neighbour to try at all (a choice that does not depend on anything but the string).  No shortcut for odd components is taken, so `nodes`
 * is exactly the number of tries of the stated order.  c1cc[nH]c1, c1ccoc1, O=c1cccc[nH]1, [O-][n+]1ccccc1 and c1cc[cH-]c1 resolve;
 * c1ccnc1 is DSP_KEKULE (where = 4, nodes = 4).  Matched aromatic bonds become order 2, the other aromatic bonds order 1.
 *
 * Hydrogens.  A bracket atom has the hydrogens it states.  A bare upper-case atom has the writer's count (diffspectra_smiles.h): the smallest
 * of the valences C 4, N 3 or 5, O 2, F 1 that is >= its bond-order sum, minus that sum; 0 if none is large enough.  A bare lower-case atom
 * has max(V - sigma - (1 if matched), 0).
 *
 * Record.  The atoms of the string first, in string order, then the hydrogens, one after the other in the order of the atoms that carry
 * them (the order of tests/smiles_mirror.parse); each such hydrogen has type 0, charge 0 and one bond of order 1.  More than 29 atoms in
 * all is DSP_TOO_LARGE (where = -1).  Positions and pad are zero, the bond block is symmetric, fields at the DS_REC_* offsets.
 *
 * Order of the statuses.  DSP_TOO_LONG, DSP_EMPTY; then the first error of the text (DSP_SYNTAX, DSP_ELEMENT); then more than 29 string atoms
 * (DSP_TOO_LARGE); then DSP_UNDECIDED / DSP_KEKULE; then more than 29 atoms with the hydrogens (DSP_TOO_LARGE).
 *
 * Stated deviations.  Not RDKit's reader: no sanitisation or valence check (diffspectra_valence.h does that on the record), stereo marks,
 * isotopes and classes are dropped, ':' between upper-case atoms is accepted, a lower-case atom outside every ring is accepted when it
 * wants nothing ([nH2]C is not refused).  Two spellings of 2-methylpyridine (Cc1ccccn1, n1ccccc1C) give the two Kekule drawings: the reader
 * makes one defined choice per string; ds_mobile / aromaticity-level identity do not see the difference.
 *
 * Method.  One wave per string, DSP_WAVES strings per workgroup, no workgroup barrier.  The row is staged in LDS with dword loads.  The
 * tokenizer is serial in lane 0 (<= 384 bytes; bracket atoms, a branch stack of <= 192 entries, a 100-entry ring table and the bond list, of
 * which a closing ring number searches the earlier entries, all in LDS).  Everything after it has an atom per lane: the bond codes go into a
 * 29 x 32 byte matrix, ring bonds come from ds_perceive::ring_bond (bounded mask growth over neighbour words), the wanting atoms from a
 * ballot; the Kekule search runs in lane 0 on neighbour masks with its stack (<= 15 levels) in LDS; hydrogens are placed by a wave prefix
 * sum; the record is assembled in LDS and leaves as whole dwords.  Integers only, no atomics, no scratch.  Every loop is bounded by the row
 * length, the bond count (<= 383), 29 atoms or max_nodes.  A row's outputs do not depend on the batch and are bit-identical from run to run;
 * a wave of the last workgroup without a string writes nothing.
 */
#ifndef DIFFSPECTRA_READER_H
#define DIFFSPECTRA_READER_H

#include <stdint.h>

#include "diffspectra_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DSP_OK 0
#define DSP_EMPTY 1
#define DSP_SYNTAX 2
#define DSP_ELEMENT 3
#define DSP_KEKULE 4
#define DSP_TOO_LARGE 5
#define DSP_UNDECIDED 6
#define DSP_TOO_LONG 7
#define DSP_TEXT_BYTES 384            /* largest stride of a text row (= DSL_TEXT_BYTES) */
#define DSP_WAVES 4                   /* strings per workgroup */
#define DSP_FLAG_ISOTOPE 1            /* bits of `flags`: read and ignored ... */
#define DSP_FLAG_CHIRAL 2
#define DSP_FLAG_DIRECTION 4
#define DSP_FLAG_CLASS 8
#define DSP_FLAG_AROMATIC 16          /* ... and: the string has lower-case atoms */

/* Records of SMILES strings.  Outputs, one row per string, every byte of every row written:
 *   rec [P, DS_RECORD_BYTES] u8   the record; all zero unless status = DSP_OK
 *   n [P] i32                     atoms of the record; 0 unless DSP_OK
 *   status [P] u8                 DSP_OK .. DSP_TOO_LONG
 *   where [P] i32                 offset of the first offending byte (DSP_SYNTAX, DSP_ELEMENT, DSP_KEKULE), else -1
 *   string_atoms [P] i32          atoms written in the string: for DSP_OK, DSP_TOO_LARGE, DSP_KEKULE, DSP_UNDECIDED; else 0
 *   flags [P] u32                 DSP_FLAG_* bits of the whole string, for the same four statuses; else 0
 *   aromatic [P] u32              bit i = record atom i was written in lower case; 0 unless DSP_OK
 *   atom_pos [P, 29] i32          offset of record atom i's symbol; -1 for the appended hydrogens, for atoms >= n and unless DSP_OK
 *   nodes [P] i32                 tries of the Kekule search (0 when it did not run)
 * DS_ERR_ARG, checked in this order: max_nodes outside [0, DS_GRAPH_MAX_NODES], P outside [0, 2^31 - 1] or a stride that is not a multiple of
 * 4 in [4, DSP_TEXT_BYTES]; then, for P > 0: a NULL text or length; a text that is not 4-byte aligned; a NULL output; a rec that is not 4-byte
 * aligned. */
int dsp_read_smiles(const uint8_t* text, int32_t stride, const int32_t* length, int64_t P, int32_t max_nodes, uint8_t* rec, int32_t* n,
                    uint8_t* status, int32_t* where, int32_t* string_atoms, uint32_t* flags, uint32_t* aromatic, int32_t* atom_pos,
                    int32_t* nodes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DIFFSPECTRA_READER_H */
