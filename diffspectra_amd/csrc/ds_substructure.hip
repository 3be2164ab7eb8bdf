// diffspectra_amd - substructure queries on result records: every pattern of a table against every record, with the number of distinct atom
// sets, the anchors and the covered atoms of its embeddings, plus the aromatic atoms, the aromatic cycle count and the fragments of the record.
// include/diffspectra_substructure.h states every definition (the matched graph, the per-atom properties, the eight bond classes, the pattern
// words, the search order and its node count); DESIGN.md section 20 has the figures.
//
// One wave64 per record, DSQ_WAVES per workgroup, an atom per lane.  The prologue runs once per record on the perception of ds_perceive.h (the
// record scan, applied_charge and max_valence, the fold test, ring_bond for every bond, reach for the fragments, the electron rule, the wave
// reductions), with the cycle walk in its other form: a lane walks the cycles through its OWN atom (not only those it is the lowest atom of),
// so that it learns its aromatic-bond neighbours without a scatter, and it keeps the distinct atom sets of the cycles it is the lowest atom
// of.  LDS holds, per wave, the bond matrix, the neighbour masks of the perception, the eight class masks of every atom, the pattern in flight with one ballot per
// pattern atom, and the lanes' search stacks (candidate mask and image per depth) at [depth * 32 + lane]: lanes 0..28 of one depth row sit on
// 29 different banks, and a dynamically indexed register array would go to scratch.  The waves of a workgroup walk the K patterns together
// (workgroup barriers around the staging of a pattern); the searches between two barriers diverge freely.  Integers only, no atomics, no
// early exit: a wave without a record takes part in the barriers and writes nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/diffspectra_substructure.h"
#include "ds_perceive.h"
#include "ds_host.h"   // DST_CHECK_LAUNCH

namespace {

using namespace ds_perceive;
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
  const unsigned me = lane < 32 ? 1u << lane : 0u;
  // the cycles through this lane's atom; those it is the lowest atom of feed the ring count
  Smallest rings;
  const Matched M = matched_graph(S.adj, S.any, S.matched, S.electrons, mine, n, lane, [&](unsigned members) {
    if (!(members & (me - 1u))) rings.insert(members);
  });
  const bool usable = M.usable, node = M.node;
  const int t = M.t, q = M.q;
  const unsigned nb = M.nb, matchable = M.matchable, ring_nb = M.ring_nb, arom_nb = M.arom_nb;
  const int X = __popc(nb) + M.hi, Ht = __popc(nb & M.isH) + M.hi;

  // fragments: the lowest atom a matchable atom reaches in the matched graph is its own in one atom per component
  unsigned lowest = me;
  if (node) {
    const unsigned reached = reach(S.matched, me, me, 0u);
    lowest = reached & (0u - reached);
  }
  const int fragments = __popc(low32(__ballot(node && lowest == me)));
  const unsigned aromatic = low32(__ballot(arom_nb != 0u));
  const int n_rings = distinct_capped(rings);

  // the eight class masks of this atom and its property word
  if (lane < 32) {
    const unsigned keep = node ? matchable : 0u, plain = keep & ~arom_nb;
    const unsigned kind[4] = {M.nb1 & plain, M.nb2 & plain, M.nb3 & plain, arom_nb & keep};
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
static_assert(PA <= 14 && DSQ_WORD_ATOM + PA <= DSQ_WORD_LINK && DSQ_WORD_LINK + PA <= DSQ_WORD_CLOSURE &&
                  DSQ_WORD_CLOSURE + DSQ_MAX_CLOSURES <= DSQ_PATTERN_WORDS,
              "the pattern's fields fit its words");
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
