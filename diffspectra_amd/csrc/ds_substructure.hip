// diffspectra_amd - substructure queries on result records: every pattern of a table against every record, with the number of distinct atom
// sets, the anchors and the covered atoms of its embeddings, plus the aromatic atoms, the aromatic cycle count and the fragments of the record.
// include/diffspectra_substructure.h states every definition (the matched graph, the per-atom properties, the eight bond classes, the pattern
// words, the search order and its node count); DESIGN.md section 20 has the figures.
//
// One wave64 per record, DSQ_WAVES per workgroup, an atom per lane.  The prologue runs once per record and restates the perception of
// ds_groups.hip with two additions: a lane walks the cycles through its OWN atom (not only those it is the lowest atom of), so that it learns
// its aromatic-bond neighbours without a scatter, and it keeps the distinct atom sets of the cycles it is the lowest atom of.  LDS holds, per
// wave, the bond matrix, the neighbour masks of the perception, the eight class masks of every atom, the pattern in flight with one ballot per
// pattern atom, and the lanes' search stacks (candidate mask and image per depth) at [depth * 32 + lane]: lanes 0..28 of one depth row sit on
// 29 different banks, and a dynamically indexed register array would go to scratch.  The waves of a workgroup walk the K patterns together
// (workgroup barriers around the staging of a pattern); the searches between two barriers diverge freely.  Integers only, no atomics, no
// early exit: a wave without a record takes part in the barriers and writes nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/diffspectra_substructure.h"
#include "ds_bonds.h"
#include "ds_records.h"
#include "ds_host.h"   // DST_CHECK_LAUNCH

namespace {

using ds_rec::MA;
using ds_rec::uniform_i;
constexpr unsigned ALL = ~0u;             // keep mask of ds_rec::load_bonds
constexpr int MAX_ORDER = 3, MAX_TYPE = 4;
constexpr int H = 0, C = 1, N = 2, O = 3, F = 4;
constexpr unsigned NONE = 3u;             // electron code of "no candidate"
constexpr int NO_PARTNER = 31;
constexpr unsigned EMPTY = ~0u;           // a slot of a "four smallest" list that holds nothing: above every atom mask
constexpr int PA = DSQ_MAX_PATTERN_ATOMS;

struct Wave {                             // one record's staging area
  unsigned char adj[MA * 32];             // symmetric bond orders over original atom indices, diagonal 0
  unsigned any[32];                       // bit j = bonded to atom j by any order
  unsigned matched[32];                   // the same among matchable atoms, 0 for a folded hydrogen
  unsigned electrons[32];                 // bits 0-1: count with the partner in the cycle, 2-3: with it outside, 4-8: the partner
  unsigned cls[8 * 32];                   // [class * 32 + atom]: the matchable neighbours over a bond of that class
  unsigned pattern[DSQ_PATTERN_WORDS];    // the pattern in flight
  unsigned fits[16];                      // [k]: the record atoms that satisfy pattern atom k
  unsigned cand[PA * 32];                 // [depth * 32 + lane]: the candidates not yet tried
  unsigned img[PA * 32];                  // [depth * 32 + lane]: the record atom assigned
};

__device__ __forceinline__ unsigned low32(unsigned long long ballot) { return (unsigned)ballot; }   // atoms live in lanes 0..28

__device__ __forceinline__ unsigned wave_or(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v |= (unsigned)__shfl_xor((int)v, o, 64);
  return (unsigned)uniform_i((int)v);
}

__device__ __forceinline__ unsigned wave_min(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, (unsigned)__shfl_xor((int)v, o, 64));
  return (unsigned)uniform_i((int)v);
}

// The four smallest distinct values a lane has seen, ascending; named members, so they stay in registers.
struct Smallest {
  unsigned s0 = EMPTY, s1 = EMPTY, s2 = EMPTY, s3 = EMPTY;
  __device__ __forceinline__ void insert(unsigned v) {
    if (v == s0 || v == s1 || v == s2 || v >= s3) return;
    if (v < s0) { s3 = s2; s2 = s1; s1 = s0; s0 = v; }
    else if (v < s1) { s3 = s2; s2 = s1; s1 = v; }
    else if (v < s2) { s3 = s2; s2 = v; }
    else s3 = v;
  }
  __device__ __forceinline__ unsigned above(unsigned prev) const {               // the lane's smallest value above `prev`; atom sets are never 0
    if (s0 > prev) return s0;
    if (s1 > prev) return s1;
    if (s2 > prev) return s2;
    return s3 > prev ? s3 : EMPTY;
  }
};

// The number of distinct values over all lanes, saturating at 4: the four smallest of the wave are among the lanes' four smallest.  Called by
// the whole wave.
__device__ __forceinline__ int distinct_capped(const Smallest& mine) {
  int count = 0;
  unsigned prev = 0u;
#pragma unroll
  for (int r = 0; r < DSQ_COUNT_CAP; ++r) {
    const unsigned next = wave_min(mine.above(prev));
    if (next == EMPTY) break;                                                     // wave-uniform
    prev = next;
    ++count;
  }
  return count;
}

__device__ __forceinline__ bool six_electrons(const Wave& S, unsigned members) {
  unsigned sum = 0u;
  bool all = true;
  for (unsigned m = members; m; m &= m - 1u) {                                   // 5 or 6 members
    const unsigned w = S.electrons[__ffs((int)m) - 1];
    const unsigned e = ((members >> (w >> 4)) & 1u) ? (w & 3u) : ((w >> 2) & 3u);
    all &= e != NONE;
    sum += e;
  }
  return all && sum == 6u;
}

// the matchable atoms that atom `a` reaches over a bond whose class lies in `set`
__device__ __forceinline__ unsigned reached_by(const Wave& S, int a, unsigned set) {
  unsigned m = 0u;
  for (unsigned s = set & 0xffu; s; s &= s - 1u) m |= S.cls[(__ffs((int)s) - 1) * 32 + a];
  return m;
}

struct Record {                           // what the prologue leaves: wave-uniform but `props`
  unsigned matchable, aromatic, props;    // props: this lane's atom as one bit per property field, 0 when it is not matchable
  int rings, fragments;
  bool usable;
};

// Holds three workgroup barriers, which every wave of the workgroup reaches.  n = 0: a wave without a record; `mine` is not touched.
__device__ __forceinline__ Record prologue(Wave& S, const unsigned char* __restrict__ mine, int n, int lane) {
  const bool active = lane < n;
  int type = 0, raw = 0;
  if (active) {
    type = mine[DS_REC_TYPE + lane];
    raw = (int)(signed char)mine[DS_REC_FC + lane];
  }
  bool bad = type > MAX_TYPE;
  const int t = min(type, MAX_TYPE);
  if (n > 0) ds_rec::load_bonds(S.adj, mine, ALL, lane);
  __syncthreads();
  int val = 0;
  unsigned nb = 0u, nb1 = 0u, nb2 = 0u, nb3 = 0u;
  if (active)
    for (int j = 0; j < n; ++j) {
      const unsigned b = S.adj[lane * 32 + j];
      bad |= b > (unsigned)MAX_ORDER;
      val += (int)b;
      nb |= (b ? 1u : 0u) << j;
      nb1 |= (b == 1u ? 1u : 0u) << j;
      nb2 |= (b == 2u ? 1u : 0u) << j;
      nb3 |= (b == 3u ? 1u : 0u) << j;
    }
  const bool usable = n > 0 && __ballot(active && bad) == 0ull;
  const bool on = usable && active;
  if (!on) nb = nb1 = nb2 = nb3 = 0u;     // an unusable record has no atoms from here on

  const unsigned isH = low32(__ballot(on && t == H)), isN = low32(__ballot(on && t == N)), isO = low32(__ballot(on && t == O));
  const int q = ((t == C || t == N) && (raw == 1 || raw == -1)) || (t == O && raw == -1) ? raw : 0;
  const int vmax = ds_bonds::c_valence[t] + (t == C ? -abs(q) : (t == N || t == O) ? q : 0);
  const int hi = max(0, vmax - val);
  const int D = __popc(nb), dbl = __popc(nb2), trp = __popc(nb3);
  const int X = D + hi, Ht = __popc(nb & isH) + hi;
  const bool folded = on && t == H && raw == 0 && D == 1 && nb1 == nb && !(nb & isH);
  const unsigned matchable = low32(__ballot(on && !folded));
  const unsigned me = lane < 32 ? 1u << lane : 0u;
  const bool node = (matchable & me) != 0u;
  if (lane < 32) {
    S.any[lane] = nb;
    S.matched[lane] = node ? nb & matchable : 0u;
  }
  __syncthreads();

  // ring bonds: neighbour j is reached without the bond to it; every atom is expanded once per neighbour
  unsigned ring_nb = 0u;
  for (unsigned left = nb; left; left &= left - 1u) {
    const unsigned goal = left & (0u - left);
    unsigned todo = nb & ~goal, reached = me | todo;
    while (todo && !(reached & goal)) {
      const int j = __ffs((int)todo) - 1;
      todo &= todo - 1u;
      const unsigned fresh = S.any[j] & ~reached;
      reached |= fresh;
      todo |= fresh;
    }
    if (reached & goal) ring_nb |= goal;
  }
  // fragments: the lowest atom a matchable atom reaches in the matched graph is its own in one atom per component
  unsigned lowest = me;
  if (node) {
    unsigned todo = me, reached = me;
    while (todo) {
      const int j = __ffs((int)todo) - 1;
      todo &= todo - 1u;
      const unsigned fresh = S.matched[j] & ~reached;
      reached |= fresh;
      todo |= fresh;
    }
    lowest = reached & (0u - reached);
  }
  const int fragments = __popc(low32(__ballot(node && lowest == me)));

  unsigned e_in = NONE, e_out = NONE;
  int partner = NO_PARTNER;
  if (on && trp == 0 && dbl <= 1 && X <= 3) {
    if (dbl == 1) {
      if ((t == C && X == 3 && q == 0) || (t == N && ((X == 2 && q == 0) || (X == 3 && q == 1)))) {
        e_in = 1u;
        partner = __ffs((int)nb2) - 1;
        e_out = (ring_nb & nb2) ? 1u : (((isN | isO) >> partner) & 1u) ? 0u : NONE;
      }
    } else if (t == C) {
      if (X == 3 && q == -1) e_in = e_out = 2u;
      else if (X == 3 && q == 1) e_in = e_out = 0u;
    } else if (t == N) {
      if ((X == 3 && q == 0) || (X == 2 && q == -1)) e_in = e_out = 2u;
    } else if (t == O) {
      if (X == 2 && q == 0) e_in = e_out = 2u;
    }
  }
  if (lane < 32) S.electrons[lane] = e_in | (e_out << 2) | ((unsigned)partner << 4);
  __syncthreads();
  const unsigned candidates = low32(__ballot(e_in != NONE));

  // cycles of 5 and 6 atoms through this lane's atom over candidates (at most three neighbours each: 3 * 2 * 2 * 2 * 2 partial paths), each
  // taken in the direction whose last atom is above its second; the cycles this atom is the lowest of feed the ring count
  unsigned arom_nb = 0u;
  Smallest rings;
  if (e_in != NONE) {
    const unsigned others = candidates & ~me, below = me - 1u;
    for (unsigned c1 = nb & others; c1; c1 &= c1 - 1u) {
      const int a1 = __ffs((int)c1) - 1;
      const unsigned m1 = me | (1u << a1);
      for (unsigned c2 = S.any[a1] & others & ~m1; c2; c2 &= c2 - 1u) {
        const int a2 = __ffs((int)c2) - 1;
        const unsigned m2 = m1 | (1u << a2);
        for (unsigned c3 = S.any[a2] & others & ~m2; c3; c3 &= c3 - 1u) {
          const int a3 = __ffs((int)c3) - 1;
          const unsigned m3 = m2 | (1u << a3);
          for (unsigned c4 = S.any[a3] & others & ~m3; c4; c4 &= c4 - 1u) {
            const int a4 = __ffs((int)c4) - 1;
            const unsigned m4 = m3 | (1u << a4), n4 = S.any[a4];
            if ((n4 & me) && a4 > a1 && six_electrons(S, m4)) {
              arom_nb |= (1u << a1) | (1u << a4);
              if (!(m4 & below)) rings.insert(m4);
            }
            for (unsigned c5 = n4 & others & ~m4; c5; c5 &= c5 - 1u) {
              const int a5 = __ffs((int)c5) - 1;
              const unsigned m5 = m4 | (1u << a5);
              if ((S.any[a5] & me) && a5 > a1 && six_electrons(S, m5)) {
                arom_nb |= (1u << a1) | (1u << a5);
                if (!(m5 & below)) rings.insert(m5);
              }
            }
          }
        }
      }
    }
  }
  const unsigned aromatic = low32(__ballot(arom_nb != 0u));
  const int n_rings = distinct_capped(rings);

  // the eight class masks of this atom and its property word
  if (lane < 32) {
    const unsigned keep = node ? matchable : 0u, plain = keep & ~arom_nb;
    const unsigned kind[4] = {nb1 & plain, nb2 & plain, nb3 & plain, arom_nb & keep};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      S.cls[k * 32 + lane] = kind[k] & ~ring_nb;
      S.cls[(k + 4) * 32 + lane] = kind[k] & ring_nb;
    }
  }
  const unsigned props = !node ? 0u
                               : (1u << (DSQ_BIT_ELEMENT + 2 * t + (arom_nb ? 1 : 0))) | (1u << (DSQ_BIT_HT + min(Ht, 4))) | (1u << (DSQ_BIT_X + min(X, 4))) |
                                     (1u << (DSQ_BIT_D + min((int)__popc(nb & matchable), 4))) | (1u << (DSQ_BIT_RING + (ring_nb ? 1 : 0))) |
                                     (1u << (DSQ_BIT_CHARGE + q + 1));
  return {usable ? matchable : 0u, usable ? aromatic : 0u, props, usable ? n_rings : 0, usable ? fragments : 0, usable};
}

struct Hits {                             // what one lane's search recorded
  Smallest sets;
  unsigned cover = 0u;
  bool any = false, stopped = false;
  __device__ __forceinline__ void record(unsigned atoms) {
    sets.insert(atoms);
    cover |= atoms;
    any = true;
  }
};

// the candidates of pattern atom k for this lane's search: satisfy it, bonded as the link wants to the image of the parent, unused, and
// bonded as every closure that ends at k wants
__device__ __forceinline__ unsigned candidates_of(const Wave& S, int k, unsigned used, int lane, int closures) {
  const unsigned link = S.pattern[DSQ_WORD_LINK + k];
  unsigned m = S.fits[k] & ~used & reached_by(S, (int)S.img[(link & 0xffu) * 32 + lane], link >> 8);
  for (int c = 0; c < closures; ++c) {
    const unsigned w = S.pattern[DSQ_WORD_CLOSURE + c];
    if ((int)((w >> 8) & 0xffu) == k) m &= reached_by(S, (int)S.img[(w & 0xffu) * 32 + lane], w >> 16);
  }
  return m;
}

// The search of the header from this lane's atom; `atoms` pattern atoms (2..14), checked by the caller together with the parents and closures.
__device__ __forceinline__ void search(Wave& S, Hits& hits, int atoms, int closures, int max_nodes, int lane) {
  unsigned used = 1u << lane;
  int k = 1, nodes = 0;
  S.img[lane] = (unsigned)lane;
  S.cand[32 + lane] = candidates_of(S, 1, used, lane, closures);
  while (k >= 1) {                                                                // at most 2 * max_nodes + 14 rounds
    const unsigned left = S.cand[k * 32 + lane];
    if (!left) {
      if (--k >= 1) used &= ~(1u << S.img[k * 32 + lane]);
      continue;
    }
    const int a = __ffs((int)left) - 1;
    S.cand[k * 32 + lane] = left & (left - 1u);
    ++nodes;
    if (k == atoms - 1) hits.record(used | (1u << a));
    else {
      S.img[k * 32 + lane] = (unsigned)a;
      used |= 1u << a;
      ++k;
      S.cand[k * 32 + lane] = candidates_of(S, k, used, lane, closures);
    }
    if (nodes >= max_nodes) {
      hits.stopped = true;
      break;
    }
  }
}

__global__ __launch_bounds__(64 * DSQ_WAVES) void k_substructure(const unsigned char* __restrict__ rec, const int32_t* __restrict__ n_atoms, int64_t P,
                                                                  const int32_t* __restrict__ patterns, int K, int max_nodes,
                                                                  unsigned char* __restrict__ count, int32_t* __restrict__ anchors,
                                                                  int32_t* __restrict__ cover, int32_t* __restrict__ aromatic_mask,
                                                                  int32_t* __restrict__ aromatic_rings, int32_t* __restrict__ fragments,
                                                                  unsigned char* __restrict__ status) {
  __shared__ Wave W[DSQ_WAVES];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * DSQ_WAVES + wave;
  const bool live = p < P;
  const int n = live ? ds_rec::atoms_of(n_atoms, p) : 0;
  Wave& S = W[wave];
  const Record r = prologue(S, rec + (live ? p : 0) * DS_RECORD_BYTES, n, lane);
  if (live && lane == 0) {
    aromatic_mask[p] = (int32_t)r.aromatic;
    aromatic_rings[p] = r.rings;
    fragments[p] = r.fragments;
    status[p] = (unsigned char)(r.usable ? DSQ_OK : DSQ_UNUSABLE);
  }
  const bool node = lane < 32 && ((r.matchable >> lane) & 1u);
  for (int e = 0; e < K; ++e) {                                                   // K is the same for every wave: the barriers are uniform
    __syncthreads();                                                              // the searches of the pattern before are over (and the class masks written)
    if (lane < DSQ_PATTERN_WORDS) S.pattern[lane] = (unsigned)patterns[(int64_t)e * DSQ_PATTERN_WORDS + lane];
    __syncthreads();
    const int atoms = (int)(S.pattern[0] & 0xffu), closures = (int)((S.pattern[0] >> 8) & 0xffu);
    bool formed = atoms >= 1 && atoms <= PA && closures <= DSQ_MAX_CLOSURES;
    if (formed) {                                                                 // wave-uniform: every lane reads the same words
      for (int k = 1; k < atoms; ++k) formed &= (int)(S.pattern[DSQ_WORD_LINK + k] & 0xffu) < k;
      for (int c = 0; c < closures; ++c) {
        const unsigned w = S.pattern[DSQ_WORD_CLOSURE + c];
        const int a = (int)(w & 0xffu), b = (int)((w >> 8) & 0xffu);
        formed &= a < b && b < atoms;
      }
    }
    Hits hits;
    if (formed) {
      for (int k = 0; k < atoms; ++k) {
        const unsigned fit = low32(__ballot(__popc(S.pattern[DSQ_WORD_ATOM + k] & r.props) == 6));
        if (lane == 0) S.fits[k] = fit;
      }
    }
    __syncthreads();
    if (formed && node && ((S.fits[0] >> lane) & 1u)) {
      if (atoms == 1) hits.record(1u << lane);
      else search(S, hits, atoms, closures, max_nodes, lane);
    }
    const int distinct = distinct_capped(hits.sets);
    const unsigned anchored = low32(__ballot(hits.any)), covered = wave_or(hits.cover);
    const bool truncated = __ballot(hits.stopped) != 0ull;
    if (live && lane == 0) {
      const int64_t at = p * K + e;
      count[at] = (unsigned char)(distinct | (truncated ? DSQ_TRUNCATED : 0));
      anchors[at] = (int32_t)anchored;
      cover[at] = (int32_t)covered;
    }
  }
}

static_assert(DSQ_WAVES >= 1 && 64 * DSQ_WAVES <= 1024, "a workgroup of whole waves");
static_assert(MA <= 29 && PA <= 14 && DSQ_WORD_ATOM + PA <= DSQ_WORD_LINK && DSQ_WORD_LINK + PA <= DSQ_WORD_CLOSURE &&
                  DSQ_WORD_CLOSURE + DSQ_MAX_CLOSURES <= DSQ_PATTERN_WORDS,
              "atom masks fit 32 bits; the pattern's fields fit its words");
static_assert(DSQ_BIT_CHARGE + 3 <= 32 && DSQ_COUNT_CAP == 4 && DSQ_COUNT_CAP < DSQ_TRUNCATED, "six property fields in one word; four slots per lane");

}  // namespace

extern "C" int dsq_match_records(const uint8_t* rec, const int32_t* n, int64_t P, const int32_t* patterns, int32_t K, int32_t max_nodes, uint8_t* count,
                                 int32_t* anchors, int32_t* cover, int32_t* aromatic_mask, int32_t* aromatic_rings, int32_t* fragments, uint8_t* status,
                                 void* stream) {
  const bool scalars = K >= 0 && K <= DSQ_MAX_PATTERNS && max_nodes >= 1 && max_nodes <= DSQ_MAX_NODES;
  const int go = ds_rec::check_table(scalars, P, rec, n, {aromatic_mask, aromatic_rings, fragments, status});
  if (go != ds_rec::LAUNCH) return go;
  if (K > 0 && (!patterns || !count || !anchors || !cover || (reinterpret_cast<uintptr_t>(patterns) & 3))) return DS_ERR_ARG;
  hipLaunchKernelGGL(k_substructure, dim3((unsigned)((P + DSQ_WAVES - 1) / DSQ_WAVES)), dim3(64 * DSQ_WAVES), 0, (hipStream_t)stream, rec, n, P, patterns,
                     (int)K, (int)max_nodes, count, anchors, cover, aromatic_mask, aromatic_rings, fragments, status);
  return DST_CHECK_LAUNCH();
}
