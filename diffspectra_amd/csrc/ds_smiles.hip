// diffspectra_amd - canonical SMILES of result records: the text that the reference gets from Chem.MolToSmiles, without RDKit.
// include/diffspectra_smiles.h states every definition (written graph, label key, signature order, target cell, twins, budget, certificate,
// writer, overflow); DESIGN.md section 19 has the method and the figures.
//
// One wave64 per record, DSL_WAVES records per workgroup, an atom per lane (lanes 0..28; a folded hydrogen keeps its lane and takes no part).
// Every wave works on its own LDS area and its loops have their own trip counts, so there is no workgroup barrier anywhere: the lanes of a
// wave are ordered by ds_refine::Wave, and a wave without a record leaves at once.  The refinement is the single-molecule form of
// ds_refine.h; the search is the iteration of k_graph_identity with one molecule: a stack of colourings in LDS, a cursor and the tried atoms
// per level.  The walk over the canonical graph and the emission run in lane 0.  Integers only, no atomics.  From ds_perceive.h: the record
// scan (with the wave barrier), the plain-hydrogen fold test, the wave minimum.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/diffspectra_smiles.h"
#include "ds_perceive.h"
#include "ds_host.h"   // DST_CHECK_LAUNCH

namespace {

using namespace ds_perceive;
using ds_refine::DISCRETE;
constexpr int TOKEN = 12;                 // an atom's text is at most "[" X "H" dd sign ddd "]" = 10 bytes
constexpr int TEXT_WORDS = DSL_TEXT_BYTES / 4;
constexpr unsigned short FREE = 0xffffu, PENDING = 0xfffeu;

struct Mol {                              // one record's staging area
  unsigned char adj[MA * 32];             // symmetric bond bytes of the WRITTEN graph over record indices, diagonal 0
  unsigned long long sig[32], f[32];      // ds_refine: signatures being ranked, per-atom colour hash of the running round
  unsigned char stack[MA][32];            // colours of every open level before its individualisation; after the search: the bond bytes in
                                          // canonical positions, canon[p * 32 + q]
  int cell[32], cursor[32];               // per level: the colour of the cell that is split, the next record index to try
  unsigned tried[32];                     // per level: the atoms individualised so far
  unsigned char inv[32], best[32];        // atom of a canonical position: at this leaf, at the best leaf so far
  unsigned char token[32][TOKEN], token_len[32];   // atom text by record index
  signed char vis[32], parent[32];        // by canonical position: visit index, parent in the walk (-1: a root)
  unsigned char order[32];                // position of the k-th visited atom
  unsigned char frame_atom[32], frame_next[32], frame_paren[32];   // the walk's stack
  unsigned short slot[DSL_MAX_RINGS + 1]; // ring number -> opening position << 8 | partner position, FREE, or PENDING until the atom ends
  int result[2];                          // length, status: lane 0's verdict for the wave
  unsigned text[TEXT_WORDS];
  __device__ __forceinline__ const unsigned char* bonds(int) const { return adj; }
};

// The walk and the emission, by one lane: m written atoms in canonical positions with the bond bytes canon[p * 32 + q].  Leaves W.vis (the
// visit index of every position) and the text; returns its length, or -1 when more than DSL_MAX_RINGS numbers would be open at once.  Every
// loop is bounded by m, m * m or DSL_MAX_RINGS.
__device__ int write_text(Mol& W, int m) {
  const unsigned char* __restrict__ canon = &W.stack[0][0];
  unsigned char* __restrict__ out = reinterpret_cast<unsigned char*>(W.text);
  int len = 0;
  auto emit = [&](int ch) {
    if (len < DSL_TEXT_BYTES) out[len] = (unsigned char)ch;
    ++len;
  };
  auto number = [&](int k) {
    if (k >= 10) { emit('%'); emit('0' + k / 10); }
    emit('0' + k % 10);
  };
  auto symbol = [&](int order) {
    if (order == 2) emit('=');
    if (order == 3) emit('#');
  };
  // the visit order: depth first from the lowest unvisited position, neighbours in ascending position
  for (int p = 0; p < m; ++p) { W.vis[p] = -1; W.parent[p] = -1; }
  int count = 0;
  for (int root = 0; root < m; ++root) {
    if (W.vis[root] >= 0) continue;
    int sp = 0;
    W.frame_atom[0] = (unsigned char)root; W.frame_next[0] = 0;
    W.vis[root] = (signed char)count; W.order[count++] = (unsigned char)root;
    while (sp >= 0) {
      const int a = W.frame_atom[sp];
      int b = W.frame_next[sp];
      while (b < m && !(canon[a * 32 + b] && W.vis[b] < 0)) ++b;
      if (b < m) {
        W.frame_next[sp] = (unsigned char)(b + 1);
        W.parent[b] = (signed char)a;
        W.vis[b] = (signed char)count; W.order[count++] = (unsigned char)b;
        ++sp;                                                        // (sp <= m - 1: a path holds every atom once)
        W.frame_atom[sp] = (unsigned char)b; W.frame_next[sp] = 0;
      } else {
        --sp;
      }
    }
  }
  // the text
  for (int k = 0; k <= DSL_MAX_RINGS; ++k) W.slot[k] = FREE;
  int top = 0;                                                       // the highest number in use so far
  bool over = false;
  auto ring = [&](int a, int b) { return canon[a * 32 + b] && W.parent[a] != b && W.parent[b] != a; };
  auto enter = [&](int a) {
    const int atom = W.best[a];
    for (int k = 0; k < W.token_len[atom]; ++k) emit(W.token[atom][k]);
    for (int t = 0; t < W.vis[a]; ++t) {                             // closures, in the partners' visit order
      const int b = W.order[t];
      if (!ring(a, b)) continue;
      const unsigned short want = (unsigned short)(b << 8 | a);
      for (int k = 1; k <= top; ++k)
        if (W.slot[k] == want) { number(k); W.slot[k] = PENDING; break; }
    }
    for (int t = W.vis[a] + 1; t < m && !over; ++t) {                // openings
      const int b = W.order[t];
      if (!ring(a, b)) continue;
      int k = 1;
      while (k <= DSL_MAX_RINGS && W.slot[k] != FREE) ++k;
      if (k > DSL_MAX_RINGS) { over = true; break; }
      W.slot[k] = (unsigned short)(a << 8 | b);
      top = max(top, k);
      symbol(canon[a * 32 + b]);
      number(k);
    }
    for (int k = 1; k <= top; ++k)
      if (W.slot[k] == PENDING) W.slot[k] = FREE;
  };
  bool first = true;
  for (int root = 0; root < m && !over; ++root) {
    if (W.parent[root] >= 0) continue;
    if (!first) emit('.');
    first = false;
    int sp = 0;
    W.frame_atom[0] = (unsigned char)root; W.frame_next[0] = 0; W.frame_paren[0] = 0;
    enter(root);
    while (sp >= 0 && !over) {
      const int a = W.frame_atom[sp];
      int b = W.frame_next[sp];
      while (b < m && W.parent[b] != a) ++b;
      if (b < m) {
        int later = b + 1;
        while (later < m && W.parent[later] != a) ++later;
        const bool last = later >= m;
        W.frame_next[sp] = (unsigned char)(b + 1);
        if (!last) emit('(');
        symbol(canon[a * 32 + b]);
        ++sp;
        W.frame_atom[sp] = (unsigned char)b; W.frame_next[sp] = 0; W.frame_paren[sp] = last ? 0 : 1;
        enter(b);
      } else {
        if (W.frame_paren[sp]) emit(')');
        --sp;
      }
    }
  }
  return over ? -1 : len;
}

__global__ __launch_bounds__(64 * DSL_WAVES) void k_smiles(const unsigned char* __restrict__ rec, const int32_t* __restrict__ n_atoms, int64_t P,
                                                           int max_nodes, unsigned char* __restrict__ text, int32_t* __restrict__ length,
                                                           unsigned char* __restrict__ status, int32_t* __restrict__ nodes,
                                                           int32_t* __restrict__ atom_order) {
  __shared__ Mol S[DSL_WAVES];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * DSL_WAVES + wave;
  if (p >= P) return;                                                // a wave without a record: no barrier below waits for it
  const ds_refine::Wave sync{};
  const int n = uniform_i(ds_rec::atoms_of(n_atoms, p));
  const unsigned char* __restrict__ mine = rec + p * DS_RECORD_BYTES;
  Mol& W = S[wave];
  const unsigned me = lane < 32 ? 1u << lane : 0u;

  for (int w = lane; w < TEXT_WORDS; w += 64) W.text[w] = 0u;
  const Atom A = scan(W.adj, mine, n, lane, sync);
  const bool active = A.active, usable = usable_record(A, n);
  const int type = A.type, fc = A.raw & 0xff;                        // the charge byte as the label key holds it
  const unsigned nb = A.nb;                                          // bonded by any order

  int out_length = 0, out_status = DSL_UNUSABLE, used = 0, place = -1;
  if (usable) {
    // the written graph: fold the plain hydrogens into their neighbours, by ballots
    const unsigned hydrogens = low32(__ballot(active && type == H));
    const int only = nb ? __ffs((int)nb) - 1 : 0;
    const bool fold = plain_hydrogen(active, type, A.raw, nb, hydrogens) && W.adj[lane * 32 + only] == 1;
    const unsigned folded = low32(__ballot(fold));
    const unsigned written = low32(__ballot(active)) & ~folded;
    const bool on = (written & me) != 0u;
    const int m = __popc(written);
    const int h = __popc(nb & folded);
    sync();                                                          // every lane has read its row
    if (fold) { W.adj[lane * 32 + only] = 0; W.adj[only * 32 + lane] = 0; }
    sync();
    int sum = 0;
    if (on)
      for (int j = 0; j < n; ++j) sum += W.adj[lane * 32 + j];

    // the atom's text
    if (on) {
      const int charge = A.raw;
      const int implied = type == 1 ? (sum <= 4 ? 4 - sum : 0) : type == 2 ? (sum <= 3 ? 3 - sum : sum <= 5 ? 5 - sum : 0)
                        : type == 3 ? (sum <= 2 ? 2 - sum : 0) : type == 4 ? (sum <= 1 ? 1 - sum : 0) : 0;
      const unsigned char sym = type == 0 ? 'H' : type == 1 ? 'C' : type == 2 ? 'N' : type == 3 ? 'O' : 'F';
      unsigned char* T = W.token[lane];
      int L = 0;
      if (type != 0 && charge == 0 && h == implied) {
        T[L++] = sym;
      } else {
        T[L++] = '[';
        T[L++] = sym;
        if (h >= 1) {
          T[L++] = 'H';
          if (h >= 10) T[L++] = (unsigned char)('0' + h / 10);
          if (h >= 2) T[L++] = (unsigned char)('0' + h % 10);
        }
        if (charge != 0) {
          const int a = charge < 0 ? -charge : charge;
          T[L++] = charge > 0 ? '+' : '-';
          if (a >= 100) T[L++] = (unsigned char)('0' + a / 100);
          if (a >= 10) T[L++] = (unsigned char)('0' + a / 10 % 10);
          if (a >= 2) T[L++] = (unsigned char)('0' + a % 10);
        }
        T[L++] = ']';
      }
      W.token_len[lane] = (unsigned char)L;
    }

    // initial colour: the rank of the label key; then the stable colouring
    const unsigned long long key = (unsigned long long)((4 - type) << 16 | fc << 8 | h);
    int colour = ds_refine::rank_jointly<false>(W, on ? key : ~0ull, n, lane, sync).colour;
    if (!on) colour = 0;
    unsigned long long multi = 0ull;
    int st = ds_refine::refine<false>(W, colour, on, n, lane, multi, sync);

    // the search: every leaf's certificate against the best so far
    int depth = 0;                                                   // open levels: W.stack[0 .. depth-1]
    bool have = false, stopped = false;
    for (int it = 0; it <= max_nodes + MA; ++it) {                   // every pass but the last spends one individualisation
      if (st == DISCRETE) {
        if (on) W.inv[colour & 31] = (unsigned char)lane;
        sync();
        bool better = !have;
        if (have) {                                                  // a lane per row of the triangle
          bool differs = false, less = false;
          if (lane < m) {
            const int a = W.inv[lane], b = W.best[lane];
            for (int q = lane + 1; q < m; ++q) {
              const unsigned x = W.adj[a * 32 + W.inv[q]], y = W.adj[b * 32 + W.best[q]];
              if (x != y) { differs = true; less = x < y; break; }
            }
          }
          const unsigned long long rows = __ballot(differs), lower = __ballot(less);
          if (rows) better = (lower >> (__ffsll((long long)rows) - 1)) & 1ull;
        }
        sync();                                                      // every lane has read W.best
        if (better) {
          place = colour;
          if (lane < m) W.best[lane] = W.inv[lane];
          have = true;
        }
        sync();
      } else {
        if (depth >= MA) break;                                      // (cannot happen: every level makes one more atom a cell of its own)
        // open a level on the lowest cell with several atoms
        const int c = (int)wave_min((on && ((multi >> lane) & 1ull)) ? (unsigned)colour : 64u);
        if (lane < 32) W.stack[depth][lane] = (unsigned char)colour;
        if (lane == 0) { W.cell[depth] = c; W.cursor[depth] = 0; W.tried[depth] = 0u; }
        sync();
        ++depth;
      }
      // the next atom to individualise: the lowest untried atom, not a twin of a tried one, of the deepest level that has one
      int u = -1, c = 0;
      unsigned tried = 0u;
      while (depth > 0) {                                            // at most 29 levels
        const int f = depth - 1;
        c = uniform_i(W.cell[f]);
        tried = (unsigned)uniform_i((int)W.tried[f]);
        const int from = uniform_i(W.cursor[f]);
        colour = lane < 32 ? W.stack[f][lane] : 0;
        unsigned cand = low32(__ballot(on && colour == c && lane >= from));
        while (cand && u < 0) {                                      // at most 29 candidates, at most 28 tried atoms each
          const int v = __ffs((int)cand) - 1;
          cand &= cand - 1u;
          bool twin = false;
          for (unsigned t = tried; t && !twin; t &= t - 1u) {
            const int w = __ffs((int)t) - 1;
            const bool same = !on || lane == v || lane == w || W.adj[v * 32 + lane] == W.adj[w * 32 + lane];
            twin = __ballot(!same) == 0ull;
          }
          if (!twin) u = v;
        }
        if (u >= 0) break;
        --depth;
      }
      if (u < 0) break;                                              // nothing left to try anywhere: the search is complete
      if (have && used >= max_nodes) { stopped = true; break; }      // the budget does not cover this one: the best leaf so far stands
      ++used;
      sync();                                                        // every lane has read the level
      if (lane == 0) { W.cursor[depth - 1] = u + 1; W.tried[depth - 1] = tried | 1u << u; }
      if (on && colour == c && lane != u) colour = c + 1;
      sync();
      st = ds_refine::refine<false>(W, colour, on, n, lane, multi, sync);
    }

    out_status = DSL_OVERFLOW;                                       // (also a search that never reached a leaf, which cannot happen)
    if (have) {
      // the bond bytes in canonical positions, then the walk and the text in lane 0
      unsigned char* canon = &W.stack[0][0];
      if (lane < m) {
        const int a = W.best[lane];
        for (int q = 0; q < m; ++q) canon[lane * 32 + q] = W.adj[a * 32 + W.best[q]];
      }
      sync();
      if (lane == 0) {
        const int len = write_text(W, m);
        const bool fits = len >= 0 && len <= DSL_TEXT_BYTES;
        W.result[0] = fits ? len : 0;
        W.result[1] = !fits ? DSL_OVERFLOW : stopped ? DSL_UNCERTIFIED : DSL_OK;
      }
      sync();
      out_length = uniform_i(W.result[0]);
      out_status = uniform_i(W.result[1]);
      place = on && out_status != DSL_OVERFLOW ? (int)W.vis[place & 31] : -1;
    } else {
      place = -1;
    }
  }

  const bool text_ok = out_status == DSL_OK || out_status == DSL_UNCERTIFIED;
  uint32_t* __restrict__ row = reinterpret_cast<uint32_t*>(text + p * DSL_TEXT_BYTES);
  for (int w = lane; w < TEXT_WORDS; w += 64) row[w] = text_ok ? W.text[w] : 0u;
  if (lane < MA) atom_order[p * MA + lane] = text_ok ? place : -1;
  if (lane == 0) {
    length[p] = out_length;
    status[p] = (unsigned char)out_status;
    nodes[p] = used;
  }
}

static_assert(DSL_WAVES >= 1 && 64 * DSL_WAVES <= 1024, "a workgroup of whole waves");
static_assert(DSL_TEXT_BYTES % 4 == 0, "the text leaves as whole dwords");
static_assert(MA * 32 <= (int)sizeof(((Mol*)nullptr)->stack), "the canonical bond bytes fit the search stack");

}  // namespace

extern "C" int dsl_smiles_records(const uint8_t* rec, const int32_t* n, int64_t P, int32_t max_nodes, uint8_t* text, int32_t* length,
                                  uint8_t* status, int32_t* nodes, int32_t* atom_order, void* stream) {
  const int go = ds_rec::check_table(max_nodes >= 0 && max_nodes <= DS_GRAPH_MAX_NODES, P, rec, n, {text, length, status, nodes, atom_order});
  if (go != ds_rec::LAUNCH) return go;
  if (reinterpret_cast<uintptr_t>(text) & 3) return DS_ERR_ARG;
  hipLaunchKernelGGL(k_smiles, dim3((unsigned)((P + DSL_WAVES - 1) / DSL_WAVES)), dim3(64 * DSL_WAVES), 0, (hipStream_t)stream, rec, n, P,
                     (int)max_nodes, text, length, status, nodes, atom_order);
  return DST_CHECK_LAUNCH();
}
