// diffspectra_amd - result records from SMILES strings: the text the reference hands to Chem.MolFromSmiles, without RDKit.
// include/diffspectra_reader.h states every definition (language, first error, aromatic bonds, the order of the Kekule search, hydrogens,
// the record); DESIGN.md section 27 has the method and the figures.
//
// One wave64 per string, DSP_WAVES strings per workgroup.  Every wave works on its own LDS area and its loops have their own trip counts,
// so there is no workgroup barrier anywhere: the lanes of a wave are ordered by ds_refine::Wave, and a wave without a string leaves at once.
// The tokenizer and the Kekule search are serial in lane 0; the graph between them and the record after them have an atom per lane.
// Integers only, no atomics.  From ds_perceive.h: ring_bond, low32.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/diffspectra_reader.h"
#include "ds_perceive.h"
#include "ds_host.h"   // DST_CHECK_LAUNCH

namespace {

using ds_perceive::low32;
using ds_rec::MA;
using ds_rec::uniform_i;
constexpr int TEXT_WORDS = DSP_TEXT_BYTES / 4, REC_WORDS = DS_RECORD_BYTES / 4;
constexpr int MAX_BONDS = DSP_TEXT_BYTES, MAX_DEPTH = DSP_TEXT_BYTES / 2, RING_NUMBERS = 100, LEVELS = 16;
constexpr int SOFT = 4;                   // bond code of ':' and of an unwritten bond: aromatic or single, decided by the graph
enum Need { NOTHING = 0, AFTER_BOND = 1, AFTER_OPEN = 2, AFTER_DOT = 3 };
enum Result { R_STATUS, R_WHERE, R_ATOMS, R_FLAGS, R_BONDS, R_NODES, R_MATCHED, R_COUNT };

struct Row {                              // one string's staging area
  unsigned text[TEXT_WORDS];
  unsigned bonds[MAX_BONDS];              // atom a | atom b << 9 | code << 18, in the order of the text
  unsigned stack[MAX_DEPTH];              // open branches: atom before '(' | offset of '(' << 9
  unsigned ring[RING_NUMBERS];            // 0 = free, else 1 + (atom | code << 9 | offset << 12)
  unsigned char type[32], hcount[32];     // of the first 29 atoms; hcount 255 = a bare atom
  signed char charge[32];
  short pos[32];
  unsigned char adj[MA * 32];             // bond codes, then bond orders, among the string's atoms; symmetric
  unsigned nbr[32], arom_nbr[32];         // neighbours by any bond, by an aromatic bond
  unsigned char mate[32], level_atom[LEVELS], level_cursor[LEVELS], level_tries[LEVELS];
  int result[R_COUNT];                    // lane 0's verdicts for the wave
  unsigned rec[REC_WORDS];
};

__device__ __forceinline__ bool is_digit(int c) { return c >= '0' && c <= '9'; }
__device__ __forceinline__ bool is_lower(int c) { return c >= 'a' && c <= 'z'; }
__device__ __forceinline__ bool is_upper(int c) { return c >= 'A' && c <= 'Z'; }
__device__ __forceinline__ int element(int c) { return c == 'H' ? 0 : c == 'C' ? 1 : c == 'N' ? 2 : c == 'O' ? 3 : c == 'F' ? 4 : -1; }

// The tokenizer, by one lane: L bytes of R.text.  Leaves the atoms, the bond list and R.result[R_STATUS .. R_BONDS].  Every loop is bounded by L,
// the bond count or RING_NUMBERS.
__device__ void tokenize(Row& R, int L) {
  const unsigned char* __restrict__ t = reinterpret_cast<const unsigned char*>(R.text);
  auto at = [&](int j) { return j < L ? (int)t[j] : -1; };          // -1: the end of the text
  for (int k = 0; k < RING_NUMBERS; ++k) R.ring[k] = 0u;
  int atoms = 0, bonds = 0, depth = 0, flags = 0, last = -1, pending = 0, need = -1, kind = NOTHING, unclosed = -1;
  int status = DSP_OK, where = -1, i = 0;
  while (i < L && status == DSP_OK && unclosed < 0) {
    const int c = t[i];
    int typ = -1, charge = 0, h = 255, pos = i, next = i + 1;
    bool arom = false;
    if (c == '[') {
      int j = i + 1, f = flags, bad = -1;                            // bad: the offending offset, L for the end of the text
      auto refuse = [&](int k) { if (bad < 0) bad = k < L ? k : L; };
      if (is_digit(at(j))) {
        f |= DSP_FLAG_ISOTOPE;
        while (is_digit(at(j))) ++j;
      }
      const int s = at(j);
      if (s < 0) {
        refuse(j);
      } else if (is_upper(s)) {
        if (is_lower(at(j + 1)) || element(s) < 0) { status = DSP_ELEMENT; where = j; }
        typ = element(s);
      } else if (s == 'c' || s == 'n' || s == 'o') {
        typ = element(s - 32);
        arom = true;
      } else if (s == 'b' || s == 's' || s == 'p' || s == '*') {
        status = DSP_ELEMENT; where = j;
      } else {
        refuse(j);
      }
      pos = j;
      if (status == DSP_OK && bad < 0) {
        ++j;
        if (at(j) == '@') {
          f |= DSP_FLAG_CHIRAL;
          ++j;
          if (at(j) == '@') ++j;
        }
        h = 0;
        if (at(j) == 'H') {
          h = 1;
          ++j;
          if (is_digit(at(j))) { h = at(j) - '0'; ++j; }
        }
        if (at(j) == '+' || at(j) == '-') {
          const int sign_at = j, sign = at(j) == '+' ? 1 : -1;
          ++j;
          if (at(j) == at(sign_at)) {
            charge = 2 * sign;
            ++j;
          } else if (is_digit(at(j))) {
            int size = 0;
            for (int d = 0; d < 3 && is_digit(at(j)); ++d, ++j) size = size * 10 + at(j) - '0';
            if (size > 127) refuse(sign_at);
            charge = sign * size;
          } else {
            charge = sign;
          }
        }
        if (bad < 0 && at(j) == ':') {
          f |= DSP_FLAG_CLASS;
          ++j;
          if (!is_digit(at(j))) refuse(j);
          while (is_digit(at(j))) ++j;
        }
        if (at(j) != ']') refuse(j);
        next = j + 1;
      }
      if (status == DSP_OK && bad >= 0) {
        if (bad >= L) { unclosed = i; need = -1; }
        else { status = DSP_SYNTAX; where = bad; }
      }
      if (status != DSP_OK || unclosed >= 0) break;
      flags = f;
    } else if (c == 'C' || c == 'N' || c == 'O' || c == 'F' || c == 'c' || c == 'n' || c == 'o') {
      if (c == 'C' && at(i + 1) == 'l') { status = DSP_ELEMENT; where = i; break; }
      arom = c >= 'a';
      typ = element(arom ? c - 32 : c);
    } else if (c == 'B' || c == 'S' || c == 'P' || c == 'I' || c == 'b' || c == 's' || c == 'p' || c == '*') {
      status = DSP_ELEMENT; where = i; break;
    } else if (c == '-' || c == '=' || c == '#' || c == ':' || c == '/' || c == '\\') {
      if (pending || last < 0) { status = DSP_SYNTAX; where = i; break; }
      if (c == '/' || c == '\\') flags |= DSP_FLAG_DIRECTION;
      pending = c == '=' ? 2 : c == '#' ? 3 : c == ':' ? SOFT : 1;
      need = i;
      kind = kind == AFTER_OPEN ? AFTER_OPEN : AFTER_BOND;
      ++i;
      continue;
    } else if (is_digit(c) || c == '%') {
      int k = c - '0';
      if (c == '%') {
        if (!(is_digit(at(i + 1)) && is_digit(at(i + 2)))) { status = DSP_SYNTAX; where = i; break; }
        k = (at(i + 1) - '0') * 10 + at(i + 2) - '0';
        next = i + 3;
      }
      if (last < 0 || kind == AFTER_OPEN || kind == AFTER_DOT) { status = DSP_SYNTAX; where = i; break; }
      const unsigned open = R.ring[k];
      if (open) {
        const int other = (int)((open - 1u) & 511u), code = (int)(((open - 1u) >> 9) & 7u);
        bool bad = other == last || (code && pending && code != pending);
        const unsigned ab = (unsigned)other | (unsigned)last << 9, ba = (unsigned)last | (unsigned)other << 9;
        for (int b = 0; b < bonds && !bad; ++b) {
          const unsigned have = R.bonds[b] & 0x3ffffu;
          bad = have == ab || have == ba;
        }
        if (bad || bonds >= MAX_BONDS) { status = DSP_SYNTAX; where = i; break; }   // (bonds: cannot happen, every bond has a byte of its own)
        R.bonds[bonds++] = ab | (unsigned)(code ? code : pending) << 18;
        R.ring[k] = 0u;
      } else {
        R.ring[k] = 1u + ((unsigned)last | (unsigned)pending << 9 | (unsigned)i << 12);
      }
      pending = 0; need = -1; kind = NOTHING;
      i = next;
      continue;
    } else if (c == '(') {
      if (last < 0 || pending || kind == AFTER_OPEN || kind == AFTER_DOT || depth >= MAX_DEPTH) { status = DSP_SYNTAX; where = i; break; }
      R.stack[depth++] = (unsigned)last | (unsigned)i << 9;
      need = i; kind = AFTER_OPEN;
      ++i;
      continue;
    } else if (c == ')') {
      if (depth == 0 || need >= 0) { status = DSP_SYNTAX; where = i; break; }
      last = (int)(R.stack[--depth] & 511u);
      ++i;
      continue;
    } else if (c == '.') {
      if (last < 0 || need >= 0 || depth) { status = DSP_SYNTAX; where = i; break; }
      last = -1; need = i; kind = AFTER_DOT;
      ++i;
      continue;
    } else {
      status = DSP_SYNTAX; where = i; break;
    }
    // an atom
    if (arom) flags |= DSP_FLAG_AROMATIC;
    if (atoms < 32) {
      R.type[atoms] = (unsigned char)typ;
      R.charge[atoms] = (signed char)charge;
      R.hcount[atoms] = (unsigned char)h;
      R.pos[atoms] = (short)(arom ? -pos - 1 : pos);                 // lower case: the offset as -pos - 1
    }
    if (last >= 0 && bonds < MAX_BONDS) R.bonds[bonds++] = (unsigned)last | (unsigned)atoms << 9 | (unsigned)pending << 18;
    last = atoms++;
    pending = 0; need = -1; kind = NOTHING;
    i = next;
  }
  if (status == DSP_OK) {                                            // what the end of the text leaves open: the lowest offset
    int open = unclosed >= 0 ? unclosed : L;
    if (need >= 0) open = min(open, need);
    if (depth) open = min(open, (int)(R.stack[0] >> 9));
    for (int k = 0; k < RING_NUMBERS; ++k)
      if (R.ring[k]) open = min(open, (int)((R.ring[k] - 1u) >> 12));
    if (open < L) { status = DSP_SYNTAX; where = open; }
  }
  R.result[R_STATUS] = status;
  R.result[R_WHERE] = where;
  R.result[R_ATOMS] = atoms;
  R.result[R_FLAGS] = flags;
  R.result[R_BONDS] = bonds;
}

// The Kekule search, by one lane: the first perfect matching of `want` along R.arom_nbr in the header's order.  Leaves R.mate and
// R.result[R_STATUS, R_WHERE, R_NODES, R_MATCHED].  Bounded by max_nodes tries; a level is undone at most once per try.
__device__ void kekulize(Row& R, unsigned want, int max_nodes) {
  unsigned matched = 0u;
  int nodes = 0, fail = -1, depth = 0, status = DSP_OK;
  while (status == DSP_OK) {
    const unsigned open = want & ~matched;
    if (!open || depth >= LEVELS) break;                             // (depth: cannot happen, 29 atoms are 14 pairs and one open level)
    R.level_atom[depth] = (unsigned char)(__ffs((int)open) - 1);
    R.level_cursor[depth] = 0;
    R.level_tries[depth] = 0;
    ++depth;
    for (bool placed = false; !placed && status == DSP_OK;) {
      const int u = R.level_atom[depth - 1], cursor = R.level_cursor[depth - 1];
      const unsigned cand = R.arom_nbr[u] & want & ~matched & (cursor >= 32 ? 0u : ~0u << cursor);
      if (cand) {
        if (nodes >= max_nodes) { status = DSP_UNDECIDED; break; }
        ++nodes;
        const int v = __ffs((int)cand) - 1;
        R.level_cursor[depth - 1] = (unsigned char)(v + 1);
        R.level_tries[depth - 1] = 1;
        matched |= 1u << u | 1u << v;
        R.mate[u] = (unsigned char)v;
        R.mate[v] = (unsigned char)u;
        placed = true;
      } else {
        if (!R.level_tries[depth - 1]) fail = u;
        if (--depth == 0) { status = DSP_KEKULE; break; }
        const int w = R.level_atom[depth - 1];
        matched &= ~(1u << w | 1u << R.mate[w]);
      }
    }
  }
  R.result[R_STATUS] = status;
  if (status == DSP_KEKULE) {
    const int p = R.pos[fail & 31];
    R.result[R_WHERE] = p < 0 ? -p - 1 : p;
  }
  R.result[R_NODES] = nodes;
  R.result[R_MATCHED] = (int)matched;
}

__device__ __forceinline__ int valence_of(int type, int charge) {
  return type == 1 ? (charge == 0 ? 4 : (charge == 1 || charge == -1) ? 3 : 0)
       : type == 2 ? (charge == 0 ? 3 : charge == 1 ? 4 : charge == -1 ? 2 : 0)
       : type == 3 ? (charge == 0 ? 2 : charge == 1 ? 3 : 0) : 0;
}

__global__ __launch_bounds__(64 * DSP_WAVES) void k_read_smiles(const unsigned char* __restrict__ text, int stride, const int32_t* __restrict__ length,
                                                                int64_t P, int max_nodes, unsigned char* __restrict__ rec, int32_t* __restrict__ n_out,
                                                                unsigned char* __restrict__ status_out, int32_t* __restrict__ where_out,
                                                                int32_t* __restrict__ string_atoms, uint32_t* __restrict__ flags_out,
                                                                uint32_t* __restrict__ aromatic_out, int32_t* __restrict__ atom_pos,
                                                                int32_t* __restrict__ nodes_out) {
  __shared__ Row S[DSP_WAVES];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * DSP_WAVES + wave;
  if (p >= P) return;                                                // a wave without a string: no barrier below waits for it
  const ds_refine::Wave sync{};
  Row& R = S[wave];
  const int L = uniform_i(length[p]);

  int status = L < 0 || L > stride ? DSP_TOO_LONG : L == 0 ? DSP_EMPTY : DSP_OK;
  int where = -1, atoms = 0, flags = 0, nodes = 0, n = 0, my_pos = -1;
  unsigned aromatic = 0u;
  for (int w = lane; w < REC_WORDS; w += 64) R.rec[w] = 0u;
  if (status == DSP_OK) {
    const uint32_t* __restrict__ src = reinterpret_cast<const uint32_t*>(text + p * stride);
    for (int w = lane; w < (L + 3) / 4; w += 64) R.text[w] = src[w];  // (L + 3) / 4 <= stride / 4: inside the row
    sync();
    if (lane == 0) tokenize(R, L);
    sync();
    status = uniform_i(R.result[R_STATUS]);
    where = uniform_i(R.result[R_WHERE]);
    if (status == DSP_OK) {
      atoms = uniform_i(R.result[R_ATOMS]);
      flags = uniform_i(R.result[R_FLAGS]);
      if (atoms > MA) status = DSP_TOO_LARGE;
    }
  }
  if (status == DSP_OK) {
    // the bond codes as a matrix, the neighbour words
    const int bonds = uniform_i(R.result[R_BONDS]);
    for (int w = lane; w < MA * 32 / 4; w += 64) reinterpret_cast<unsigned*>(R.adj)[w] = 0u;
    sync();
    for (int b = lane; b < bonds; b += 64) {                          // no two bonds share a pair, so no two lanes share a byte
      const unsigned e = R.bonds[b];
      const int a = (int)(e & 511u), c = (int)((e >> 9) & 511u), code = (int)(e >> 18);
      R.adj[a * 32 + c] = R.adj[c * 32 + a] = (unsigned char)(code ? code : SOFT);
    }
    sync();
    const bool on = lane < atoms;
    const int slot = lane & 31;
    const int type = on ? R.type[slot] : 0, charge = on ? R.charge[slot] : 0, stated = on ? R.hcount[slot] : 0;
    const int raw_pos = on ? R.pos[slot] : 0;
    const bool arom = on && raw_pos < 0, bare = stated == 255;
    my_pos = on ? (raw_pos < 0 ? -raw_pos - 1 : raw_pos) : -1;
    aromatic = low32(__ballot(arom));
    unsigned nb = 0u, soft = 0u;
    if (on)
      for (int j = 0; j < atoms; ++j) {
        const unsigned b = R.adj[slot * 32 + j];
        nb |= (b ? 1u : 0u) << j;
        soft |= (b == (unsigned)SOFT ? 1u : 0u) << j;
      }
    if (lane < 32) R.nbr[lane] = nb;
    sync();
    // an unwritten bond between two lower-case atoms is aromatic iff it is a ring bond; sigma counts it 1 either way
    unsigned arom_nb = 0u;
    int sigma = 0;
    if (on) {
      for (unsigned todo = arom ? soft & aromatic : 0u; todo; todo &= todo - 1u) {
        const unsigned goal = todo & (0u - todo);
        if (ds_perceive::ring_bond(R.nbr, 1u << lane, nb, goal)) arom_nb |= goal;
      }
      for (int j = 0; j < atoms; ++j) {
        const int b = R.adj[slot * 32 + j];
        sigma += b == SOFT ? 1 : b;
      }
    }
    if (lane < 32) R.arom_nbr[lane] = arom_nb;
    const int V = valence_of(type, charge);
    const unsigned want = low32(__ballot(arom && V - sigma - (bare ? 0 : stated) >= 1));
    sync();
    if (lane == 0) kekulize(R, want, max_nodes);
    sync();
    status = uniform_i(R.result[R_STATUS]);
    nodes = uniform_i(R.result[R_NODES]);
    if (status == DSP_KEKULE) where = uniform_i(R.result[R_WHERE]);
    if (status == DSP_OK) {
      const unsigned matched = (unsigned)uniform_i(R.result[R_MATCHED]);
      const bool mine = on && ((matched >> lane) & 1u);
      const int mate = mine ? R.mate[slot] : -1;
      int sum = 0;
      if (on)
        for (int j = 0; j < atoms; ++j) {                            // the orders: every lane its own row, both halves of the matrix
          int b = R.adj[slot * 32 + j];
          if (b == SOFT) b = j == mate && ((arom_nb >> j) & 1u) ? 2 : 1;
          R.adj[slot * 32 + j] = (unsigned char)b;
          sum += b;
        }
      int h = 0;
      if (on) {
        if (!bare) h = stated;
        else if (arom) h = max(V - sigma - (mine ? 1 : 0), 0);
        else h = type == 1 ? (sum <= 4 ? 4 - sum : 0) : type == 2 ? (sum <= 3 ? 3 - sum : sum <= 5 ? 5 - sum : 0)
               : type == 3 ? (sum <= 2 ? 2 - sum : 0) : type == 4 ? (sum <= 1 ? 1 - sum : 0) : 0;
      }
      int upto = h;                                                  // inclusive prefix sum over the lanes
#pragma unroll
      for (int o = 1; o < 32; o <<= 1) {
        const int below = __shfl_up(upto, o, 64);
        if (lane >= o) upto += below;
      }
      n = atoms + uniform_i(__shfl(upto, 31, 64));
      if (n > MA) {
        status = DSP_TOO_LARGE;
      } else {
        sync();                                                      // the orders are in place
        unsigned char* __restrict__ out = reinterpret_cast<unsigned char*>(R.rec);
        if (on) {
          out[DS_REC_TYPE + lane] = (unsigned char)type;
          out[DS_REC_FC + lane] = (unsigned char)charge;
          for (int j = 0; j < atoms; ++j) out[DS_REC_BOND + lane * MA + j] = R.adj[slot * 32 + j];
          for (int k = 0, at = atoms + upto - h; k < h; ++k, ++at) {   // my hydrogens: type 0 and charge 0 are there already
            out[DS_REC_BOND + lane * MA + at] = 1;
            out[DS_REC_BOND + at * MA + lane] = 1;
          }
        }
      }
    }
  }
  sync();
  const bool ok = status == DSP_OK;
  const bool read = ok || status == DSP_TOO_LARGE || status == DSP_KEKULE || status == DSP_UNDECIDED;
  uint32_t* __restrict__ row = reinterpret_cast<uint32_t*>(rec + p * DS_RECORD_BYTES);
  for (int w = lane; w < REC_WORDS; w += 64) row[w] = ok ? R.rec[w] : 0u;
  if (lane < MA) atom_pos[p * MA + lane] = ok ? my_pos : -1;
  if (lane == 0) {
    n_out[p] = ok ? n : 0;
    status_out[p] = (unsigned char)status;
    where_out[p] = where;
    string_atoms[p] = read ? atoms : 0;
    flags_out[p] = read ? (uint32_t)flags : 0u;
    aromatic_out[p] = ok ? aromatic : 0u;
    nodes_out[p] = nodes;
  }
}

static_assert(DSP_WAVES >= 1 && 64 * DSP_WAVES <= 1024, "a workgroup of whole waves");
static_assert(DSP_TEXT_BYTES % 4 == 0 && DSP_TEXT_BYTES <= 511, "rows are read as dwords; offsets and atom indices fit nine bits");
static_assert(DS_RECORD_BYTES % 4 == 0 && MA <= 32, "the record leaves as whole dwords; an atom per lane of the lower half wave");

}  // namespace

extern "C" int dsp_read_smiles(const uint8_t* text, int32_t stride, const int32_t* length, int64_t P, int32_t max_nodes, uint8_t* rec, int32_t* n,
                               uint8_t* status, int32_t* where, int32_t* string_atoms, uint32_t* flags, uint32_t* aromatic, int32_t* atom_pos,
                               int32_t* nodes, void* stream) {
  if (max_nodes < 0 || max_nodes > DS_GRAPH_MAX_NODES || P < 0 || P > 0x7fffffffll || stride < 4 || stride > DSP_TEXT_BYTES || stride % 4) return DS_ERR_ARG;
  if (P == 0) return DS_OK;
  if (!text || !length || reinterpret_cast<uintptr_t>(text) & 3) return DS_ERR_ARG;
  for (const void* o : {(const void*)rec, (const void*)n, (const void*)status, (const void*)where, (const void*)string_atoms, (const void*)flags,
                        (const void*)aromatic, (const void*)atom_pos, (const void*)nodes})
    if (!o) return DS_ERR_ARG;
  if (reinterpret_cast<uintptr_t>(rec) & 3) return DS_ERR_ARG;
  hipLaunchKernelGGL(k_read_smiles, dim3((unsigned)((P + DSP_WAVES - 1) / DSP_WAVES)), dim3(64 * DSP_WAVES), 0, (hipStream_t)stream, text, (int)stride,
                     length, P, (int)max_nodes, rec, n, status, where, string_atoms, flags, aromatic, atom_pos, nodes);
  return DST_CHECK_LAUNCH();
}
