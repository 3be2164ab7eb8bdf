// diffspectra_amd - Fraggle analytics on result records: the fragmentations of a molecule by one, two or three cuts, the branched path
// fingerprint with per-atom bits, the atom-contribution marking and the best Tanimoto over all fragmentations, behind the "Fraggle
// similarity" line of the reference's per-pair table.  include/diffspectra_fraggle.h states every definition (atom and bond codes, the hash,
// the four kinds with their thresholds and their order, the marking with its ring step, the budget); DESIGN.md section 24 has the method
// and the figures.
//
// One wave64 per record or pair, DSF_WAVES per workgroup.  Perception is ds_perceive::matched_graph, an atom per lane; from it every lane
// keeps its atom's code and its neighbour masks in registers and the wave leaves the bond list of the graph in LDS (`Graph`: a word per bond,
// per atom the 64-bit mask of its bonds, the atom codes).  A fingerprint spreads the bond sets over the lanes: lane e takes the sets whose
// lowest bond is e and grows them, five levels of compile-time recursion with the set in registers, by the adjacent higher bonds that no
// earlier member could have added (the ESU enumeration on the line graph), so every set is met once and the count is a property of the
// graph; bits go into LDS rows with atomicOr.  The fragmentations are walked in the header's order by a wave-uniform cursor; the pieces of a
// cut come from ds_perceive::components over shuffles, "on a cycle of the piece" from ds_perceive::ring_bond on the neighbour masks without
// the cuts.  Integers only, no global atomics, no early exit before the last barrier of the perception; the loops after it run a different
// number of times in every wave and hold wave barriers only.
//
// LDS per wave: 29 x 128 B of atom bits for either molecule, five 128 B fingerprint rows, three graphs of 544 B, the perception's 1.3 KB and
// four mask rows: 11 520 B, which would let 14 workgroups of one wave share a CU; the similarity kernel's 201 VGPRs allow 8, the other two
// kernels' 104 and 107 VGPRs 16, so registers and not LDS bound the occupancy.  No scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/diffspectra_fraggle.h"
#include "ds_perceive.h"
#include "ds_host.h"   // DST_CHECK_LAUNCH

namespace {

using namespace ds_perceive;
typedef unsigned long long u64;

constexpr int ATT = 31;                   // the far end of an attachment bond: no atom (atoms live in 0..28), inc[ATT] = 0
constexpr int WORDS = DSF_FP_WORDS;
__device__ __forceinline__ void sync() { ds_refine::Wave{}(); }    // the waves of a workgroup share nothing once the perception is done

struct Graph {                            // what a fingerprint reads
  u64 inc[32];                            // bit e = bond e has an end at this atom
  unsigned bond[64];                      // lower atom | higher atom (or ATT) << 5 | class << 10
  unsigned char code[32];                 // atom codes; code[ATT] = DSF_CODE_ATTACH
};

struct Wave {                             // one pair's staging area
  unsigned char adj[MA * 32];             // the perception's: bond orders, neighbours by any order, among matchable atoms, electron words
  unsigned any[32], matched[32], electrons[32];
  unsigned kept[32];                      // Q's matchable neighbours without the cuts of the candidate at hand
  unsigned ring[32];                      // Q's neighbours over a ring bond
  unsigned nbr[2][32];                    // the matchable neighbours of Q and of R, for the ring step
  Graph g[2], f;                          // Q, R and the fragment graph
  unsigned fp[2][WORDS], a[WORDS], marked_fp[2][WORDS];
  unsigned bits[2][MA * WORDS];           // the bits of every atom of Q and of R
};

struct Mol {                              // a perceived record: what a lane keeps of its atom, and wave-uniform figures
  bool usable, node, aromatic;
  unsigned mnb, ring_m;                   // matchable neighbours / those over a ring bond
  int code;
  unsigned matchable;
  int hac, bonds;                         // bonds > DSF_MAX_BONDS: over every budget, the bond list is not complete
};

__device__ __forceinline__ u64 bit64(int e) { return 1ull << e; }

// The incidence masks of a graph whose bond list and codes are written.  Holds the wave barriers around it.
__device__ __forceinline__ void incidence(Graph& g, int bonds, int lane) {
  sync();
  if (lane < 32) {
    u64 inc = 0ull;
    if (lane < MA)
      for (int e = 0; e < bonds; ++e) {
        const unsigned w = g.bond[e];
        if ((int)(w & 31u) == lane || (int)((w >> 5) & 31u) == lane) inc |= bit64(e);
      }
    g.inc[lane] = inc;
  }
  sync();
}

// Holds the three workgroup barriers of matched_graph, which every wave of the workgroup reaches.  n = 0: a wave without a record.
__device__ __forceinline__ Mol perceive(Wave& S, Graph& g, unsigned (&nbr)[32], const unsigned char* __restrict__ mine, int n, int lane) {
  const Matched M = matched_graph(S.adj, S.any, S.matched, S.electrons, mine, n, lane, [](unsigned) {});
  const unsigned me = lane < 32 ? 1u << lane : 0u;
  const unsigned mnb = M.node ? M.nb & M.matchable : 0u;
  const bool aromatic = M.node && M.arom_nb != 0u;
  const int code = 2 * M.t + (aromatic ? 1 : 0);
  const unsigned up = lane < 32 ? mnb & ~((me << 1) - 1u) : 0u;
  const int mine_up = (int)__popc(up);
  int first = 0;
  for (int j = 0; j < n; ++j) {
    const int c = __shfl(mine_up, j, 64);
    if (j < lane) first += c;
  }
  const int bonds = wave_sum(mine_up);
  if (bonds <= DSF_MAX_BONDS) {
    int e = first;
    for (unsigned left = up; left; left &= left - 1u, ++e) {
      const int b = __ffs((int)left) - 1;
      const unsigned cls = ((M.arom_nb >> b) & 1u) ? 3u : ((M.nb1 >> b) & 1u) ? 0u : ((M.nb2 >> b) & 1u) ? 1u : 2u;
      g.bond[e] = (unsigned)lane | ((unsigned)b << 5) | (cls << 10);
    }
  }
  if (lane < 32) {
    g.code[lane] = (unsigned char)(lane == ATT ? DSF_CODE_ATTACH : M.node ? code : 0);
    nbr[lane] = mnb;
  }
  incidence(g, bonds <= DSF_MAX_BONDS ? bonds : 0, lane);
  return {M.usable, M.node, aromatic, mnb, M.node ? M.ring_nb & mnb : 0u, code, M.matchable, (int)__popc(M.matchable), bonds};
}

// ------------------------------------------------------------------------------------------------------------------ the fingerprint

struct Set {                              // a bond set in registers: every index is a compile-time constant once grow<> is unrolled
  unsigned end_a[DSF_MAX_PATH], end_b[DSF_MAX_PATH], cls[DSF_MAX_PATH], code_a[DSF_MAX_PATH], code_b[DSF_MAX_PATH];
  u64 inc_a[DSF_MAX_PATH], inc_b[DSF_MAX_PATH];
};

template <int K, bool ATOMS>
__device__ __forceinline__ void emit(const Set& s, u64 sub, unsigned* fp, unsigned* table) {
  unsigned c[K];
  unsigned atoms = 0u;
#pragma unroll
  for (int i = 0; i < K; ++i) {
    const unsigned da = (unsigned)__popcll(s.inc_a[i] & sub), db = s.end_b[i] == (unsigned)ATT ? 1u : (unsigned)__popcll(s.inc_b[i] & sub);
    const unsigned x = s.code_a[i] * 8u + da, y = s.code_b[i] * 8u + db;
    c[i] = (min(x, y) << 9) | (max(x, y) << 2) | s.cls[i];
    atoms |= 1u << s.end_a[i];
    if (s.end_b[i] != (unsigned)ATT) atoms |= 1u << s.end_b[i];
  }
#pragma unroll
  for (int i = 0; i < K - 1; ++i)
#pragma unroll
    for (int j = 0; j < K - 1 - i; ++j) {
      const unsigned lo = min(c[j], c[j + 1]), hi = max(c[j], c[j + 1]);
      c[j] = lo;
      c[j + 1] = hi;
    }
  uint64_t h = (uint64_t)K;
#pragma unroll
  for (int i = 0; i < K; ++i) h = ds_rec::mix2(h, (uint64_t)c[i]);
  const unsigned p0 = (unsigned)h & 1023u, p1 = (unsigned)(h >> 32) & 1023u;
  const unsigned w0 = p0 >> 5, m0 = 1u << (p0 & 31u), w1 = p1 >> 5, m1 = 1u << (p1 & 31u);
  atomicOr(&fp[w0], m0);
  atomicOr(&fp[w1], m1);
  if (ATOMS)
    for (; atoms; atoms &= atoms - 1u) {                                           // 2 .. 6 atoms, each below MA
      unsigned* row = table + (__ffs((int)atoms) - 1) * WORDS;
      atomicOr(&row[w0], m0);
      atomicOr(&row[w1], m1);
    }
}

// The sets that extend `sub` (K bonds, in s) by a bond of ext; closed = sub and everything adjacent to it; above = the bonds above the lowest
template <int K, bool ATOMS>
__device__ __forceinline__ void grow(const Graph& g, Set& s, u64 sub, u64 ext, u64 closed, u64 above, int& count, int max_nodes, unsigned* fp,
                                     unsigned* table) {
  while (ext && count <= max_nodes) {
    const int w = __ffsll((long long)ext) - 1;
    ext &= ext - 1ull;
    const unsigned word = g.bond[w];
    s.end_a[K] = word & 31u;
    s.end_b[K] = (word >> 5) & 31u;
    s.cls[K] = word >> 10;
    s.code_a[K] = g.code[s.end_a[K]];
    s.code_b[K] = g.code[s.end_b[K]];
    s.inc_a[K] = g.inc[s.end_a[K]];
    s.inc_b[K] = g.inc[s.end_b[K]];
    const u64 grown = sub | bit64(w);
    emit<K + 1, ATOMS>(s, grown, fp, table);
    ++count;
    if constexpr (K + 1 < DSF_MAX_PATH) {
      const u64 near = (s.inc_a[K] | s.inc_b[K]) & ~bit64(w);
      grow<K + 1, ATOMS>(g, s, grown, ext | (near & ~closed & above), closed | near, above, count, max_nodes, fp, table);
    }
  }
}

// The fingerprint of g into fp (and the atom rows into table): the number of bond sets, or -1 when there are more than max_nodes - a lane
// stops once it has met that many on its own, so every loop is bounded by the budget and the verdict does not depend on where it stopped.
template <bool ATOMS>
__device__ __forceinline__ int fingerprint(const Graph& g, int bonds, int max_nodes, unsigned* fp, unsigned* table, int lane) {
  if (lane < WORDS) fp[lane] = 0u;
  if (ATOMS)
    for (int i = lane; i < MA * WORDS; i += 64) table[i] = 0u;
  sync();
  int count = 0;
  if (lane < bonds) {
    Set s;
    const u64 above = ~((bit64(lane) << 1) - 1ull);
    grow<0, ATOMS>(g, s, 0ull, bit64(lane), bit64(lane), above, count, max_nodes, fp, table);    // the root is the one extension of the empty set
  }
  sync();
  const bool over = __ballot(count > max_nodes) != 0ull;
  const int total = wave_sum(count);                                               // <= 64 * (DSF_MAX_NODES + 1)
  return over || total > max_nodes ? -1 : total;
}

// (common, either) of two fingerprint rows
__device__ __forceinline__ void tanimoto(const unsigned* x, const unsigned* y, int lane, int& common, int& either) {
  const unsigned a = lane < WORDS ? x[lane] : 0u, b = lane < WORDS ? y[lane] : 0u;
  common = wave_sum((int)__popc(a & b));
  either = wave_sum((int)__popc(a | b));
}

// ------------------------------------------------------------------------------------------------------------------ the fragmentations

__device__ __forceinline__ int pop(u64& m) {
  const int e = __ffsll((long long)m) - 1;
  m &= m - 1ull;
  return e;
}

struct Cursor {                           // wave-uniform: where the walk through the header's order stands
  int kind, cuts, c[3];
  u64 first, second, third;
  bool probe;                             // the kind-2 test of a ring pair before its kind-3 candidates
};

__device__ __forceinline__ Cursor start(u64 chain) { return {0, 0, {0, 0, 0}, chain, 0ull, 0ull, false}; }

// The next candidate cut set: false when there is none left
__device__ __forceinline__ bool next(Cursor& k, u64 chain, u64 ring) {
  k.probe = false;
  for (;;) {
    if (k.kind == 0) {
      if (k.first) { k.c[0] = pop(k.first); k.cuts = 1; return true; }
      k.kind = 1; k.first = chain; k.second = 0ull;
    } else if (k.kind < 3) {
      if (k.second) { k.c[1] = pop(k.second); k.cuts = 2; return true; }
      if (k.first) { k.c[0] = pop(k.first); k.second = k.first; continue; }
      k.kind += 1;
      k.first = k.kind == 3 && !chain ? 0ull : ring;                                // no chain cut: no kind 3
      k.second = k.third = 0ull;
    } else {
      if (k.third) { k.c[2] = pop(k.third); k.cuts = 3; return true; }
      if (k.second) { k.c[1] = pop(k.second); k.third = chain; k.cuts = 2; k.probe = true; return true; }
      if (k.first) { k.c[0] = pop(k.first); k.second = k.first; continue; }
      return false;
    }
  }
}

struct Judged {                           // wave-uniform: the fragmentations of one candidate (two for kind 2 at the most)
  int found;
  unsigned mask0, mask1;
  int total0, total1;
  __device__ __forceinline__ unsigned mask(int i) const { return i ? mask1 : mask0; }
  __device__ __forceinline__ int total(int i) const { return i ? total1 : total0; }
};

// The pieces of Q without the candidate's cuts, judged by the rules of `kind`.  Called by the whole wave; holds wave barriers.
__device__ __forceinline__ Judged judge(Wave& S, const Mol& Q, int kind, int cuts, const int (&c)[3], int n, int lane) {
  const unsigned me = lane < 32 ? 1u << lane : 0u;
  unsigned knb = Q.mnb, ends = 0u;
  int end_a[3], end_b[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const unsigned w = k < cuts ? S.g[0].bond[c[k]] : 0u;
    end_a[k] = uniform_i((int)(w & 31u));
    end_b[k] = uniform_i((int)((w >> 5) & 31u));
    if (k < cuts) {
      if (lane == end_a[k]) knb &= ~(1u << end_b[k]);
      if (lane == end_b[k]) knb &= ~(1u << end_a[k]);
      ends |= (1u << end_a[k]) | (1u << end_b[k]);
    }
  }
  sync();                                                                          // the readers of the candidate before
  if (lane < 32) S.kept[lane] = knb;
  sync();
  const unsigned comp = components(Q.node ? knb | me : 0u, n);
  int att = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (k < cuts) att += (int)((comp >> end_a[k]) & 1u) + (int)((comp >> end_b[k]) & 1u);
  const int size = (int)__popc(comp) + att;
  const bool root = Q.node && __ffs((int)comp) - 1 == lane;
  // an atom that carries an attachment lies on a cycle of its piece iff one of its bonds there is a ring bond of the graph without the cuts
  bool cyclic = false;
  if (kind >= 2 && (ends & me))
    for (unsigned left = knb; left && !cyclic; left &= left - 1u) cyclic = ring_bond(S.kept, me, knb, left & (0u - left));
  const unsigned on_cycle = low32(__ballot(cyclic));
  const bool ringed = att == 2 && !(comp & ends & ~on_cycle) && size > 3;
  Judged out = {0, 0u, 0u, 0, 0};
  if (kind == 2) {
    const int pieces = (int)__popcll(__ballot(root));
    const unsigned valid = low32(__ballot(root && pieces == 2 && ringed && 5 * size > 2 * Q.hac));      // two roots at the most
    if (valid) {                                                                   // ascending lowest atom
      const int r = __ffs((int)valid) - 1;
      out.mask0 = (unsigned)uniform_i(__shfl((int)comp, r, 64));
      out.total0 = uniform_i(__shfl(size, r, 64));
      out.found = 1;
    }
    if (valid & (valid - 1u)) {
      const int r = 31 - __clz((int)valid);
      out.mask1 = (unsigned)uniform_i(__shfl((int)comp, r, 64));
      out.total1 = uniform_i(__shfl(size, r, 64));
      out.found = 2;
    }
  } else {
    const bool keep = Q.node && ((att == 1 && size > 3) || (kind == 3 && ringed));
    const int kept = (int)__popcll(__ballot(root && keep));
    const int total = wave_sum(root && keep ? size : 0);
    if ((kind == 3 ? kept == 2 : kept >= 1) && 5 * total > 3 * Q.hac) {
      out.found = 1;
      out.mask0 = low32(__ballot(keep));
      out.total0 = total;
    }
  }
  return out;
}

// The cut bonds of Q as masks over its bond numbers (wave-uniform): chain cuts and ring cuts
__device__ __forceinline__ void cut_bonds(const Wave& S, const Mol& Q, int lane, u64& chain, u64& ring) {
  bool is_chain = false, is_ring = false;
  if (lane < Q.bonds) {
    const unsigned w = S.g[0].bond[lane], a = w & 31u, b = (w >> 5) & 31u;
    const unsigned ra = S.ring[a], rb = S.ring[b];
    const bool ring_bond_ = (ra >> b) & 1u;
    is_chain = !ring_bond_ && (w >> 10) == 0u;
    is_ring = ring_bond_ && (__popc(ra) >= 3 || __popc(rb) >= 3);
  }
  chain = __ballot(is_chain);
  ring = __ballot(is_ring);
}

__device__ __forceinline__ unsigned pack_cuts(const Wave& S, const Cursor& k) {
  unsigned word = 0u;
#pragma unroll
  for (int i = 0; i < 3; ++i) word |= (i < k.cuts ? S.g[0].bond[k.c[i]] & 1023u : (unsigned)DSF_NO_CUT) << (10 * i);
  return word;
}

// The fragment graph of (kept, cuts) into S.f: the number of its bonds (at most one more than Q has)
__device__ __forceinline__ int fragment_graph(Wave& S, const Mol& Q, unsigned kept, const Cursor& k, int lane) {
  bool keep = false;
  unsigned w = 0u;
  if (lane < Q.bonds) {
    w = S.g[0].bond[lane];
    bool cut = false;
#pragma unroll
    for (int i = 0; i < 3; ++i) cut |= i < k.cuts && k.c[i] == lane;
    keep = !cut && ((kept >> (w & 31u)) & (kept >> ((w >> 5) & 31u)) & 1u);
  }
  const u64 real = __ballot(keep);
  sync();                                                                          // the readers of the fragment graph before
  if (keep) S.f.bond[__popcll(real & (bit64(lane) - 1ull))] = w;
  int bonds = (int)__popcll(real);
#pragma unroll
  for (int i = 0; i < 3; ++i)
    if (i < k.cuts) {
      const unsigned cw = S.g[0].bond[k.c[i]];
      for (int side = 0; side < 2; ++side) {
        const unsigned end = side ? (cw >> 5) & 31u : cw & 31u;
        if ((kept >> end) & 1u) {
          if (lane == 0) S.f.bond[bonds] = end | ((unsigned)ATT << 5) | (cw & ~1023u);
          ++bonds;
        }
      }
    }
  if (lane < 32) S.f.code[lane] = S.g[0].code[lane];                               // unmarked: marked codes are written to g and read there only
  incidence(S.f, bonds, lane);
  return bonds;
}

// ------------------------------------------------------------------------------------------------------------------ the marking

// The distance of this lane's atom from s in the graph nbr[] without the bond s-t; -1 when it is not reached.  Wave-uniform loops.
__device__ __forceinline__ int distance_from(const unsigned (&nbr)[32], int s, int t, int lane) {
  unsigned visited = 1u << s, frontier = visited;
  int mine = lane == s ? 0 : -1;
  for (int d = 1; frontier; ++d) {                                                 // every atom is expanded once
    unsigned reached = 0u;
    for (unsigned left = frontier; left; left &= left - 1u) {
      const int j = __ffs((int)left) - 1;
      unsigned to = nbr[j];
      if (j == s) to &= ~(1u << t);
      if (j == t) to &= ~(1u << s);
      reached |= to;
    }
    frontier = (unsigned)uniform_i((int)(reached & ~visited));
    visited |= frontier;
    if (lane < 32 && ((frontier >> lane) & 1u)) mine = d;
  }
  return mine;
}

// The atoms of a molecule marked against the fragment fingerprint a[]: own = the popcount of this lane's atom row
__device__ __forceinline__ unsigned mark(const Mol& X, const unsigned* table, const unsigned* a, const unsigned (&nbr)[32], int own, int lane) {
  int common = 0;
  if (lane < MA && own)
    for (int k = 0; k < WORDS; ++k) {
      const int w = (k + lane) & (WORDS - 1);                                      // skewed: the rows are 32 banks apart
      common += (int)__popc(table[lane * WORDS + w] & a[w]);
    }
  const unsigned first = low32(__ballot(X.node && own > 0 && 5 * common < 4 * own));
  unsigned marked = first;
  for (unsigned atoms = first & low32(__ballot(X.ring_m != 0u)); atoms; atoms &= atoms - 1u) {
    const int m = __ffs((int)atoms) - 1;
    for (unsigned to = (unsigned)uniform_i(__shfl((int)X.ring_m, m, 64)); to; to &= to - 1u) {
      const int x = __ffs((int)to) - 1;
      const int dm = distance_from(nbr, m, x, lane), dx = distance_from(nbr, x, m, lane);
      const int whole = uniform_i(__shfl(dm, x, 64));                              // a ring bond: x is reached without it
      marked |= low32(__ballot(dm >= 0 && dx >= 0 && dm + dx == whole));
    }
  }
  return marked;
}

__device__ __forceinline__ int row_bits(const unsigned* table, int lane) {
  int own = 0;
  if (lane < MA)
    for (int k = 0; k < WORDS; ++k) own += (int)__popc(table[lane * WORDS + ((k + lane) & (WORDS - 1))]);
  return own;
}

// ------------------------------------------------------------------------------------------------------------------ the kernels

__global__ __launch_bounds__(64 * DSF_WAVES) void k_fragmentations(const unsigned char* __restrict__ rec, const int32_t* __restrict__ n_atoms, int64_t P,
                                                                   int max_nodes, int32_t* __restrict__ rows, int32_t* __restrict__ summary,
                                                                   unsigned char* __restrict__ status) {
  __shared__ Wave W[DSF_WAVES];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * DSF_WAVES + wave;
  const bool live = p < P;
  const int n = live ? ds_rec::atoms_of(n_atoms, p) : 0;
  Wave& S = W[wave];
  const Mol Q = perceive(S, S.g[0], S.nbr[0], rec + (live ? p : 0) * DS_RECORD_BYTES, n, lane);
  if (!live) return;                                                               // behind the last workgroup barrier
  if (lane < 32) S.ring[lane] = Q.ring_m;
  const bool counted = Q.usable && Q.bonds <= DSF_MAX_BONDS && fingerprint<false>(S.g[0], Q.bonds, max_nodes, S.fp[0], nullptr, lane) >= 0;
  sync();
  int32_t* __restrict__ out = rows + p * (DSF_MAX_FRAGMENTATIONS * 4);
  int found = 0;
  u64 chain = 0ull, ring = 0ull;
  if (counted) {
    cut_bonds(S, Q, lane, chain, ring);
    Cursor k = start(chain);
    bool any2 = false;
    while (next(k, chain, ring)) {
      if (k.kind == 3 && !any2) break;                                             // no ring pair passed kind 2
      const Judged j = judge(S, Q, k.probe ? 2 : k.kind, k.cuts, k.c, n, lane);
      if (k.probe) {
        if (!j.found) k.third = 0ull;
        continue;
      }
      any2 |= k.kind == 2 && j.found > 0;
      for (int i = 0; i < j.found; ++i, ++found)
        if (found < DSF_MAX_FRAGMENTATIONS && lane < 4)
          out[found * 4 + lane] = lane == 0 ? (int32_t)j.mask(i) : lane == 1 ? (int32_t)pack_cuts(S, k) : lane == 2 ? k.kind : j.total(i);
    }
  }
  for (int i = min(found, DSF_MAX_FRAGMENTATIONS) * 4 + lane; i < DSF_MAX_FRAGMENTATIONS * 4; i += 64) out[i] = -1;
  if (lane < 4) {
    const int v = lane == 0 ? Q.hac : lane == 1 ? (int)__popcll(chain) : lane == 2 ? (int)__popcll(ring)
                                                                                     : found | (found > DSF_MAX_FRAGMENTATIONS ? DSF_TRUNCATED : 0);
    summary[p * 4 + lane] = counted ? v : 0;
  }
  if (lane == 0) status[p] = (unsigned char)(!Q.usable ? DSF_UNUSABLE : counted ? DSF_OK : DSF_UNDECIDED);
}

__global__ __launch_bounds__(64 * DSF_WAVES) void k_fingerprints(const unsigned char* __restrict__ rec, const int32_t* __restrict__ n_atoms, int64_t P,
                                                                 int max_nodes, int32_t* __restrict__ fp, int32_t* __restrict__ atom_bits,
                                                                 int32_t* __restrict__ count, unsigned char* __restrict__ status) {
  __shared__ Wave W[DSF_WAVES];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * DSF_WAVES + wave;
  const bool live = p < P;
  const int n = live ? ds_rec::atoms_of(n_atoms, p) : 0;
  Wave& S = W[wave];
  const Mol Q = perceive(S, S.g[0], S.nbr[0], rec + (live ? p : 0) * DS_RECORD_BYTES, n, lane);
  if (!live) return;
  const int sets = Q.usable && Q.bonds <= DSF_MAX_BONDS ? fingerprint<true>(S.g[0], Q.bonds, max_nodes, S.fp[0], S.bits[0], lane) : -1;
  const bool ok = sets >= 0;
  if (lane < WORDS) fp[p * WORDS + lane] = ok ? (int32_t)S.fp[0][lane] : 0;
  for (int i = lane; i < MA * WORDS; i += 64) atom_bits[p * (MA * WORDS) + i] = ok ? (int32_t)S.bits[0][i] : 0;
  if (lane == 0) {
    count[p] = ok ? sets : Q.usable ? -1 : 0;
    status[p] = (unsigned char)(!Q.usable ? DSF_UNUSABLE : ok ? DSF_OK : DSF_UNDECIDED);
  }
}

__global__ __launch_bounds__(64 * DSF_WAVES) void k_similarity(const unsigned char* __restrict__ prb_rec, const int32_t* __restrict__ prb_n, int64_t P,
                                                               const unsigned char* __restrict__ ref_rec, const int32_t* __restrict__ ref_n, int64_t M,
                                                               const int64_t* __restrict__ ref_index, int max_nodes, int32_t* __restrict__ plain,
                                                               int32_t* __restrict__ modified, int32_t* __restrict__ best_index,
                                                               int32_t* __restrict__ n_fragmentations, int32_t* __restrict__ marked,
                                                               unsigned char* __restrict__ status) {
  __shared__ Wave W[DSF_WAVES];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * DSF_WAVES + wave;
  const bool live = p < P;
  const ds_rec::Pair pair = ds_rec::pair_of(live ? p : 0, prb_rec, prb_n, ref_rec, ref_n, live ? ref_index : nullptr, live ? M : 0);
  const bool read = live && pair.valid;                                            // neither record nor count is touched otherwise
  Wave& S = W[wave];
  const int n = read ? pair.n_ref() : 0, n_r = read ? pair.n_prb() : 0;
  const Mol Q = perceive(S, S.g[0], S.nbr[0], read ? pair.ref : pair.prb, n, lane);
  const Mol R = perceive(S, S.g[1], S.nbr[1], pair.prb, n_r, lane);
  if (!live) return;                                                               // behind the last workgroup barrier
  if (lane < 32) S.ring[lane] = Q.ring_m;
  const bool usable = read && Q.usable && R.usable;
  bool decided = usable && Q.bonds <= DSF_MAX_BONDS && R.bonds <= DSF_MAX_BONDS;
  if (decided) decided = fingerprint<true>(S.g[0], Q.bonds, max_nodes, S.fp[0], S.bits[0], lane) >= 0;
  if (decided) decided = fingerprint<true>(S.g[1], R.bonds, max_nodes, S.fp[1], S.bits[1], lane) >= 0;
  int plain_c = -1, plain_e = -1, best_c = -1, best_e = -1, best = -1, found = 0;
  unsigned best_q = 0u, best_r = 0u;
  if (decided) {
    tanimoto(S.fp[0], S.fp[1], lane, plain_c, plain_e);
    const int own_q = row_bits(S.bits[0], lane), own_r = row_bits(S.bits[1], lane);
    u64 chain, ring;
    cut_bonds(S, Q, lane, chain, ring);
    Cursor k = start(chain);
    bool any2 = false;
    while (decided && next(k, chain, ring)) {
      if (k.kind == 3 && !any2) break;                                             // no ring pair passed kind 2
      const Judged j = judge(S, Q, k.probe ? 2 : k.kind, k.cuts, k.c, n, lane);
      if (k.probe) {
        if (!j.found) k.third = 0ull;
        continue;
      }
      any2 |= k.kind == 2 && j.found > 0;
      for (int i = 0; i < j.found && decided; ++i, ++found) {
        const int bonds = fragment_graph(S, Q, j.mask(i), k, lane);
        if (fingerprint<false>(S.f, bonds, max_nodes, S.a, nullptr, lane) < 0) {
          decided = false;
          break;
        }
        const unsigned mq = mark(Q, S.bits[0], S.a, S.nbr[0], own_q, lane), mr = mark(R, S.bits[1], S.a, S.nbr[1], own_r, lane);
        if (lane < MA) {
          const unsigned me = 1u << lane;
          S.g[0].code[lane] = (unsigned char)((mq & me) ? (Q.aromatic ? DSF_CODE_WILD_AROMATIC : DSF_CODE_WILD) : Q.node ? Q.code : 0);
          S.g[1].code[lane] = (unsigned char)((mr & me) ? (R.aromatic ? DSF_CODE_WILD_AROMATIC : DSF_CODE_WILD) : R.node ? R.code : 0);
        }
        sync();
        fingerprint<false>(S.g[0], Q.bonds, max_nodes, S.marked_fp[0], nullptr, lane);      // the graphs of the plain fingerprints: within the budget
        fingerprint<false>(S.g[1], R.bonds, max_nodes, S.marked_fp[1], nullptr, lane);
        int c, e;
        tanimoto(S.marked_fp[0], S.marked_fp[1], lane, c, e);
        if (best < 0 || (int64_t)c * best_e > (int64_t)best_c * e) {           // Q has bonds, so either > 0
          best = found; best_c = c; best_e = e; best_q = mq; best_r = mr;
        }
        if (lane < MA) {                                                           // the codes of Q as the next fragment graph reads them
          S.g[0].code[lane] = (unsigned char)(Q.node ? Q.code : 0);
        }
        sync();
      }
    }
  }
  if (lane == 0) {
    plain[p * 2] = decided ? plain_c : -1;
    plain[p * 2 + 1] = decided ? plain_e : -1;
    modified[p * 2] = decided && best >= 0 ? best_c : -1;
    modified[p * 2 + 1] = decided && best >= 0 ? best_e : -1;
    best_index[p] = decided ? best : -1;
    n_fragmentations[p] = decided ? found : 0;
    marked[p * 2] = decided ? (int32_t)best_q : 0;
    marked[p * 2 + 1] = decided ? (int32_t)best_r : 0;
    status[p] = (unsigned char)(!read ? DSF_INVALID : !usable ? DSF_UNUSABLE : decided ? DSF_OK : DSF_UNDECIDED);
  }
}

static_assert(DSF_WAVES >= 1 && 64 * DSF_WAVES <= 1024, "a workgroup of whole waves");
static_assert(DSF_MAX_BONDS + 1 <= 64 && MA <= ATT, "a bond per lane and per bit, the fragment graph's extra bond included; ATT is no atom");
static_assert(DSF_FP_BITS == 32 * WORDS && (WORDS & (WORDS - 1)) == 0 && DSF_MAX_PATH == 5, "the bit positions and the skew of the row reads");
static_assert((2 * 4 + 1) * 8 + 5 < 128 && DSF_CODE_WILD_AROMATIC * 8 + 5 < 128, "an end code has 7 bits");
static_assert(sizeof(Wave) * DSF_WAVES <= 64 * 1024, "static LDS of a workgroup");

inline bool budget_ok(int32_t max_nodes) { return max_nodes >= 1 && max_nodes <= DSF_MAX_NODES; }

}  // namespace

extern "C" int dsf_fraggle_fragmentations(const uint8_t* rec, const int32_t* n, int64_t P, int32_t max_nodes, int32_t* rows, int32_t* summary,
                                          uint8_t* status, void* stream) {
  const int go = ds_rec::check_table(budget_ok(max_nodes), P, rec, n, {rows, summary, status});
  if (go != ds_rec::LAUNCH) return go;
  hipLaunchKernelGGL(k_fragmentations, dim3((unsigned)((P + DSF_WAVES - 1) / DSF_WAVES)), dim3(64 * DSF_WAVES), 0, (hipStream_t)stream, rec, n, P,
                     (int)max_nodes, rows, summary, status);
  return DST_CHECK_LAUNCH();
}

extern "C" int dsf_path_fingerprints(const uint8_t* rec, const int32_t* n, int64_t P, int32_t max_nodes, int32_t* fp, int32_t* atom_bits, int32_t* count,
                                     uint8_t* status, void* stream) {
  const int go = ds_rec::check_table(budget_ok(max_nodes), P, rec, n, {fp, atom_bits, count, status});
  if (go != ds_rec::LAUNCH) return go;
  hipLaunchKernelGGL(k_fingerprints, dim3((unsigned)((P + DSF_WAVES - 1) / DSF_WAVES)), dim3(64 * DSF_WAVES), 0, (hipStream_t)stream, rec, n, P,
                     (int)max_nodes, fp, atom_bits, count, status);
  return DST_CHECK_LAUNCH();
}

extern "C" int dsf_fraggle_similarity_records(const uint8_t* prb_rec, const int32_t* prb_n, int64_t P, const uint8_t* ref_rec, const int32_t* ref_n,
                                              int64_t M, const int64_t* ref_index, int32_t max_nodes, int32_t* plain, int32_t* modified,
                                              int32_t* best_index, int32_t* n_fragmentations, int32_t* marked, uint8_t* status, void* stream) {
  const int go = ds_rec::check_pairs(budget_ok(max_nodes), P, M, prb_rec, prb_n, ref_rec, ref_n, ref_index,
                                     {plain, modified, best_index, n_fragmentations, marked, status});
  if (go != ds_rec::LAUNCH) return go;
  hipLaunchKernelGGL(k_similarity, dim3((unsigned)((P + DSF_WAVES - 1) / DSF_WAVES)), dim3(64 * DSF_WAVES), 0, (hipStream_t)stream, prb_rec, prb_n, P,
                     ref_rec, ref_n, M, ref_index, (int)max_nodes, plain, modified, best_index, n_fragmentations, marked, status);
  return DST_CHECK_LAUNCH();
}
