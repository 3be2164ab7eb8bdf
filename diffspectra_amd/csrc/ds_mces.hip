// diffspectra_amd - exact maximum-common-edge-subgraph (MCES) distance of the evaluation path: how far a generated molecule is from its
// ground truth as a labelled graph (elements and bond orders), the graded half of the reference's table next to the identity of ds_graph.hip.
// One wave64 per pair and per workgroup, integers only, no atomics, wave-uniform control flow (ds_mces_records in include/diffspectra_hip.h
// states the definition and the two deviations from the reference's number; DESIGN.md section 11 has the algorithm and the figures).
//
// Depth-first branch-and-bound over partial injective type-preserving maps pi of the generated atoms (A) into the ground-truth atoms (B).
// Soundness, in the lines the code below keeps true:
//   dist is written from `best`, and `best` only ever takes the score of a partial map that is on the stack at that moment and is copied to
//     S.best then: the returned map achieves dist, so dist is an upper bound whatever the budget;
//   a subtree is skipped only when bound <= best with bound = score + min(rem_a, rem_b) and
//     rem_a = sum of ub_A(e) over bonds e of A with an undecided end and no end decided "unmapped": any bond of A that can still add to the
//       score is one of these, and it adds min(w_e, w_f) <= ub_A(e) for the bond f of B it lands on, whose end classes are e's;
//     rem_b = sum of ub_B(f) over bonds f of B whose ends are not both used: a bond of B with both ends used has its preimage decided, so what
//       it adds is in the score already, and every other bond of B adds at most ub_B(f), once (the map is injective);
//     ub_A(e) = min(w_e, heaviest bond of B between e's end classes), ub_B likewise.  A class is the atom type, except that the eighth and all
//       later distinct types of a pair share class 7: merging classes only raises a bound, which stays admissible (QM9 has five types);
//   candidates after one with score + gain + rem_a <= best are skipped too: they are sorted by gain and rem_a does not depend on the image;
//   status EXACT is written only when the search is exhausted or best has reached the root bound min(sum ub_A, sum ub_B).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/diffspectra_hip.h"
#include "ds_records.h"
#include "ds_host.h"   // DST_CHECK_LAUNCH

namespace {

using ds_rec::MA;                         // 29 atoms: lanes 0..28 hold the generated molecule (A), lanes 32..60 the ground truth (B)
using ds_rec::uniform_i;
constexpr int NCLS = 8;                   // type classes of the bound: one byte each of a 64-bit row
constexpr unsigned NONE = 255;

struct Level {                            // an open level d of the search: the state BEFORE atom order[d] is decided
  int used;                               // ground-truth atoms taken by levels 0 .. d-1
  int score;                              // of the map of levels 0 .. d-1
  int rem_a_map, rem_a_skip;              // rem_a after order[d] is mapped (the same for every image) / after it is decided "unmapped"
  int rem_b;                              // before this level's decision: an image k takes its delta off
  int cursor, count;                      // next entry of list[d] to try (count = "unmapped", beyond = closed); number of candidates
  int pad;
};

// What a wave keeps in registers, one entry per lane, and reads with v_readlane (a lane index that is the same in every lane), so that
// a try touches LDS for its list word only:
//   lane q < depth  `decided` of level q: atom i | mapped << 5 | image m << 8 | class(m) << 16 | class(i) << 24;  `order` = atom of level q
//   lane i < 32     `ubdeg` = sum over j of ub_A(i, j);  every lane: `type`, `cls` of its own atom
struct Lanes {
  unsigned type, decided;
  int cls, order, ubdeg;
  bool keep;
  unsigned long long other;               // tab row of the OTHER side for this lane's class: what a bond of mine into class u can meet there
};

struct Search {
  unsigned char w[2][MA * 32];            // bond weights w[s][i * 32 + j] (ds_rec::load_bonds; 0 where an end is not kept), side 0 = A, 1 = B
  unsigned char cls[2][32];               // class 0..7 of every atom's type
  unsigned long long row[2][32];          // set-up: byte u of row[s][k] = heaviest bond of atom k of side s into class u
  unsigned long long tab[2][NCLS];        // byte u of tab[s][t] = heaviest bond of side s between classes t and u
  unsigned char best[32];                 // image of every atom of A in the best map (NONE: unmapped)
  Level lvl[MA];
  unsigned int list[MA][32];              // per level, sorted by gain (descending; lowest atom first): image k | gain << 5 | delta_b << 18
};

__device__ __forceinline__ unsigned byte_of(unsigned long long row, unsigned c) { return (unsigned)(row >> (8u * c)) & 255u; }

// sum over the 32 lanes of the own half (A: lanes 0..31, B: lanes 32..63)
__device__ __forceinline__ int half_sum(int v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Opens level d on atom order[d] under the partial map of levels 0 .. d-1: every lane of the B half computes the gain of its atom as the
// image and what it takes off rem_b, the candidates are ranked, and the level's scalars are left in S.lvl[d].  Returns the candidate count.
__device__ int open_level(Search& S, int d, int used, int score, int rem_a, int rem_b, const Lanes& R, int lane) {
  const int idx = lane & 31, side = lane >> 5;
  const int row_of = min(idx, MA - 1);                                     // (lanes 29..31 of a half hold no atom: any row inside the matrix)
  const int i = __builtin_amdgcn_readlane(R.order, d);
  const unsigned ti = (unsigned)__builtin_amdgcn_readlane((int)R.type, i);
  const unsigned long long tab_i = S.tab[1][__builtin_amdgcn_readlane(R.cls, i)];
  const int row_i = S.w[0][i * 32 + idx];                                  // lane j < 32: w_A(i, j)
  int gain = 0, delta = 0, to_mapped = 0, to_skipped = 0;
  for (int q = 0; q < d; ++q) {                                            // the decided atoms of A (at most 28)
    const unsigned e = (unsigned)__builtin_amdgcn_readlane((int)R.decided, q);
    const unsigned j = e & 31u, m = (e >> 8) & 31u;
    const int wa = __builtin_amdgcn_readlane(row_i, (int)j);
    const int ua = min(wa, (int)byte_of(tab_i, (e >> 24) & 7u));
    if (e & 32u) {
      const int wb = S.w[1][row_of * 32 + m];
      to_mapped += ua;
      gain += min(wa, wb);
      delta += min(wb, (int)byte_of(R.other, (e >> 16) & 7u));
    } else {
      to_skipped += ua;
    }
  }
  const bool cand = side == 1 && R.keep && !((used >> idx) & 1) && R.type == ti;
  const unsigned candidates = (unsigned)(__ballot(cand) >> 32);
  const int key = cand ? (gain << 5 | (31 - idx)) : -1;
  int rank = 0;
  for (unsigned rest = candidates; rest; rest &= rest - 1u)                // at most 29 candidates
    rank += __builtin_amdgcn_readlane(key, 32 + (__ffs(rest) - 1)) > key;
  if (cand) S.list[d][rank] = (unsigned)idx | (unsigned)gain << 5 | (unsigned)delta << 18;
  const int count = __popc(candidates);
  if (lane == 0) {
    Level L;
    L.used = used; L.score = score; L.rem_a_map = rem_a - to_mapped; L.rem_a_skip = rem_a - (__builtin_amdgcn_readlane(R.ubdeg, i) - to_skipped);
    L.rem_b = rem_b; L.cursor = 0; L.count = count; L.pad = 0;
    S.lvl[d] = L;
  }
  __syncthreads();
  return count;
}

__global__ __launch_bounds__(64) void k_mces_records(const unsigned char* __restrict__ prb_rec, const int32_t* __restrict__ prb_n,
                                                     const unsigned char* __restrict__ ref_rec, const int32_t* __restrict__ ref_n,
                                                     const int64_t* __restrict__ ref_index, int64_t M, int drop_h, int max_nodes,
                                                     int32_t* __restrict__ dist, int32_t* __restrict__ lower, unsigned char* __restrict__ status,
                                                     int32_t* __restrict__ nodes, int32_t* __restrict__ map) {
  __shared__ Search S;
  const int64_t p = blockIdx.x;
  const int lane = threadIdx.x, idx = lane & 31, side = lane >> 5;
  const ds_rec::Pair q = ds_rec::pair_of(p, prb_rec, prb_n, ref_rec, ref_n, ref_index, M);
  if (!q.valid) {
    if (lane < MA) map[p * MA + lane] = -1;
    if (lane == 0) { dist[p] = -1; lower[p] = -1; status[p] = DS_MCES_INVALID; nodes[p] = 0; }
    return;
  }
  const int n_a = q.n_prb(), n_b = q.n_ref();
  const unsigned char* __restrict__ mine = side ? q.ref : q.prb;
  const bool present = idx < (side ? n_b : n_a);
  const unsigned type = present ? mine[DS_REC_TYPE + idx] : 0u;
  const bool keep = present && !(drop_h && type == 0u);
  const unsigned long long kept = __ballot(keep);
  const int row_of = min(idx, MA - 1);
  ds_rec::load_bonds(S.w[0], q.prb, (unsigned)kept, lane);                 // a pair with an end beyond n, or a dropped hydrogen, weighs 0
  ds_rec::load_bonds(S.w[1], q.ref, (unsigned)(kept >> 32), lane);
  // class of an atom: its type's place among the pair's distinct types in order of first appearance (A before B), at most 7
  int cls = 0;
  {
    unsigned long long todo = kept;
    for (int c = 0; c < 64 && todo; ++c) {
      const unsigned t = (unsigned)__builtin_amdgcn_readlane((int)type, __ffsll((long long)todo) - 1);
      const bool same = keep && type == t;
      if (same) cls = min(c, NCLS - 1);
      todo &= ~__ballot(same);
    }
  }
  S.cls[side][idx] = (unsigned char)cls;
  S.best[idx] = (unsigned char)NONE;
  __syncthreads();
  // weighted degree; heaviest bond of every atom into every class, then of every class into every class
  int wdeg = 0;
  unsigned long long mine_row = 0ull;
  for (int j = 0; j < MA; ++j) {
    const unsigned w = S.w[side][row_of * 32 + j];
    const unsigned c = S.cls[side][j];
    wdeg += (int)w;
    if (w > byte_of(mine_row, c)) mine_row = (mine_row & ~(255ull << (8u * c))) | (unsigned long long)w << (8u * c);
  }
  if (idx >= MA) { wdeg = 0; mine_row = 0ull; }
  S.row[side][idx] = mine_row;
  __syncthreads();
  if (idx < NCLS) {
    unsigned long long acc = 0ull;
    for (int k = 0; k < MA; ++k) {
      const unsigned long long rk = S.row[side][k];
      if (S.cls[side][k] != idx) continue;                                 // (rows of atoms that are not kept are 0)
#pragma unroll
      for (unsigned c = 0; c < NCLS; ++c)
        if (byte_of(rk, c) > byte_of(acc, c)) acc = (acc & ~(255ull << (8u * c))) | (unsigned long long)byte_of(rk, c) << (8u * c);
    }
    S.tab[side][idx] = acc;
  }
  __syncthreads();
  const unsigned long long other = S.tab[side ^ 1][cls];                   // what a bond of mine into class u can meet on the other side
  int ubdeg = 0;
  for (int j = 0; j < MA; ++j) ubdeg += min((int)S.w[side][row_of * 32 + j], (int)byte_of(other, S.cls[side][j]));
  if (idx >= MA) ubdeg = 0;
  const int wsum = half_sum(wdeg), usum = half_sum(ubdeg);
  const int w_a = __builtin_amdgcn_readlane(wsum, 0) / 2, w_b = __builtin_amdgcn_readlane(wsum, 32) / 2;
  const int sum_a = __builtin_amdgcn_readlane(usum, 0) / 2, sum_b = __builtin_amdgcn_readlane(usum, 32) / 2;
  const int root = min(sum_a, sum_b);
  const int n_keep = __popc((unsigned)kept);
  // branching order of A: the atom of largest weighted degree, then the largest bond weight into the atoms already ordered
  Lanes R;
  R.type = type; R.decided = 0u; R.cls = cls; R.order = 0; R.ubdeg = ubdeg; R.keep = keep; R.other = other;
  {
    int conn = 0;
    bool ordered = false;
    for (int s = 0; s < n_keep; ++s) {
      int key = (side == 0 && keep && !ordered) ? (conn << 18 | wdeg << 5 | (31 - idx)) : -1;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) key = max(key, __shfl_xor(key, o, 64));
      const int v = 31 - (uniform_i(key) & 31);
      if (lane == s) R.order = v;
      if (lane == v) ordered = true;
      conn += S.w[0][v * 32 + idx];
    }
  }
  __syncthreads();

  int best = 0, used_nodes = 0, out = DS_MCES_EXACT;
  if (root > 0) {                                                          // (root > 0 needs a bond on each side: n_keep >= 2)
    out = DS_MCES_UNDECIDED;
    int d = 0;
    int count = open_level(S, 0, 0, 0, sum_a, sum_b, R, lane);
    int cursor = 0, l_used = 0, l_score = 0, l_rem_b = sum_b;
    int l_map = uniform_i(S.lvl[0].rem_a_map), l_skip = uniform_i(S.lvl[0].rem_a_skip);
    for (int it = 0; it < 2 * max_nodes + 64; ++it) {                      // a pass is a try (at most max_nodes) or closes a level a try opened
      if (cursor > count) {
        if (d == 0) { out = DS_MCES_EXACT; break; }                        // nothing left to try anywhere
        --d;
        const Level L = S.lvl[d];
        l_used = uniform_i(L.used); l_score = uniform_i(L.score); l_map = uniform_i(L.rem_a_map); l_skip = uniform_i(L.rem_a_skip);
        l_rem_b = uniform_i(L.rem_b); cursor = uniform_i(L.cursor); count = uniform_i(L.count);
        continue;
      }
      if (used_nodes >= max_nodes) break;                                  // the budget does not cover this try: undecided
      ++used_nodes;
      const bool mapped = cursor < count;
      const unsigned e = mapped ? (unsigned)uniform_i((int)S.list[d][cursor]) : 0u;
      const int k = e & 31u;
      const int score = l_score + (int)((e >> 5) & 8191u);
      const int rem_a = mapped ? l_map : l_skip, rem_b = l_rem_b - (int)(e >> 18);
      ++cursor;
      if (mapped && score + rem_a <= best) cursor = count;                 // no later image gains more: only "unmapped" is left here
      const bool better = score > best;
      const bool descend = d + 1 < n_keep && score + min(rem_a, rem_b) > max(best, score);
      if (better || descend) {
        const int i = __builtin_amdgcn_readlane(R.order, d);
        const unsigned e_d = (unsigned)i | (mapped ? 32u : 0u) | (unsigned)k << 8 | (unsigned)__builtin_amdgcn_readlane(R.cls, 32 + k) << 16 |
                             (unsigned)__builtin_amdgcn_readlane(R.cls, i) << 24;
        if (lane == d) R.decided = e_d;
      }
      if (better) {                                                        // the partial map on the stack is a common subgraph of its own
        best = score;
        if (lane < 32) S.best[lane] = (unsigned char)NONE;
        __syncthreads();
        if (lane <= d && (R.decided & 32u)) S.best[R.decided & 31u] = (unsigned char)((R.decided >> 8) & 31u);
        __syncthreads();
        if (best >= root) { out = DS_MCES_EXACT; break; }
      }
      if (descend) {
        if (lane == 0) S.lvl[d].cursor = cursor;
        ++d;
        l_used |= mapped ? 1 << k : 0; l_score = score; l_rem_b = rem_b;
        count = open_level(S, d, l_used, score, rem_a, rem_b, R, lane);
        cursor = 0;
        l_map = uniform_i(S.lvl[d].rem_a_map); l_skip = uniform_i(S.lvl[d].rem_a_skip);
      }
    }
  }
  if (lane < MA) {
    const unsigned m = lane < n_a ? S.best[lane] : NONE;
    map[p * MA + lane] = m == NONE ? -1 : (int)m;
  }
  if (lane == 0) {
    const int total = w_a + w_b;
    dist[p] = total - 2 * best;
    lower[p] = out == DS_MCES_EXACT ? total - 2 * best : total - 2 * root;
    status[p] = (unsigned char)out;
    nodes[p] = used_nodes;
  }
}

}  // namespace

extern "C" int ds_mces_records(const uint8_t* prb_rec, const int32_t* prb_n, int64_t P, const uint8_t* ref_rec, const int32_t* ref_n, int64_t M,
                               const int64_t* ref_index, int32_t drop_h, int32_t max_nodes, int32_t* dist, int32_t* lower, uint8_t* status,
                               int32_t* nodes, int32_t* map, void* stream) {
  const int go = ds_rec::check_pairs(max_nodes >= 0 && max_nodes <= DS_MCES_MAX_NODES && (drop_h == 0 || drop_h == 1), P, M, prb_rec, prb_n,
                                     ref_rec, ref_n, ref_index, {dist, lower, status, nodes, map});
  if (go != ds_rec::LAUNCH) return go;
  hipLaunchKernelGGL(k_mces_records, dim3((unsigned)P), dim3(64), 0, (hipStream_t)stream, prb_rec, prb_n, ref_rec, ref_n, ref_index, M,
                     (int)drop_h, (int)max_nodes, dist, lower, status, nodes, map);
  return DST_CHECK_LAUNCH();
}
