// diffspectra_amd - Morgan (ECFP-like) fingerprints of the evaluation path and the set sizes behind their Tanimoto / cosine similarity, the
// reference's "Tanimoto (Morgan)" and "Cosine (Morgan)" next to the identity of ds_graph.hip and the distance of ds_mces.hip.  One wave64 per
// molecule or per pair and per workgroup, integers only, no atomics, wave-uniform control flow (ds_morgan_records and
// ds_morgan_similarity_records in include/diffspectra_hip.h state the definition and the deviations from the reference's number; DESIGN.md
// section 12 has the method and the figures).
//
// An atom per lane: lanes 0..28 hold the generated molecule (or the only one), lanes 32..60 the ground truth; a set of atoms is a 32-bit mask.
// What the code below keeps true, in the order of the definition:
//   cycle flag    for every atom i the components of the kept graph WITHOUT i are found by squaring the reach masks (reach_j <- union of
//                 reach_k over k in reach_j; ceil(log2(atoms)) rounds close them); a bond i-j stays connected without itself exactly when
//                 j reaches another neighbour of i there, so c_i = some neighbour of i has a second neighbour of i in its component;
//   environments  E(B), the kept bonds with an end in the atom set B, is held as canon(B) = B plus every kept atom all of whose neighbours are
//                 in B.  canon(B) is the set of atoms all of whose bonds are in E(B): it depends on E(B) only, and E(canon(B)) = E(B), so
//                 E(B) = E(B') exactly when canon(B) = canon(B').  An empty E(B) is the mark EMPTY, which equals no mask;
//   features      slot r * 32 + i of a side holds the value of environment (i, r) and `ok` says whether it counts: layer 0 every kept atom,
//                 layer r >= 1 the lowest atom of every distinct new bond set, with the smallest id_r over the atoms that share the set.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/diffspectra_hip.h"
#include "ds_records.h"
#include "ds_host.h"   // DST_CHECK_LAUNCH

namespace {

using ds_rec::MA;
using ds_rec::mix2;
constexpr int SLOTS = (DS_MORGAN_MAX_RADIUS + 1) * 32;      // feature slots of a side: 32 per layer, 29 of them atoms
constexpr unsigned EMPTY = 1u << 31;                       // an environment without a bond (atoms are bits 0..28)
static_assert(SLOTS == 128 && DS_MORGAN_MAX_FEATURES == MA * (DS_MORGAN_MAX_RADIUS + 1), "two slots per lane; 29 features per layer");

struct Side {                                              // one molecule in LDS; arrays of 32 are indexed by atom
  unsigned long long feat[SLOTS];
  unsigned long long id[32];                               // id_{r-1}, then id_r, of every atom
  unsigned int nb[32];                                     // kept bonded neighbours of every atom (0 for an atom that is not kept)
  unsigned int env[DS_MORGAN_MAX_RADIUS][32];              // canon mask of E_r(i) for r = 1 .. R, or EMPTY
  unsigned char adj[MA * 32];
  unsigned char fresh[32];                                 // environment (i, r) of the running layer is new
  unsigned char ok[SLOTS], first[SLOTS];                   // the slot holds a feature; ... and no lower slot holds the same (folded) value
};

// lane k of the own half, for a k that is the same in every lane
__device__ __forceinline__ unsigned half_read(unsigned v, int k, int side) {
  const unsigned a = (unsigned)__builtin_amdgcn_readlane((int)v, k), b = (unsigned)__builtin_amdgcn_readlane((int)v, 32 + k);
  return side ? b : a;
}

__device__ __forceinline__ unsigned half_ballot(bool x, int side) {
  const unsigned long long b = __ballot(x);
  return side ? (unsigned)(b >> 32) : (unsigned)b;
}

// The feature list of the header for one molecule per half wave: S[side].feat / ok, slots 0 .. (R + 1) * 32 - 1.  rec / n of the lower and of
// the upper half; a half with n = 0 reads nothing.  Loops over atoms run over `any`, the atoms kept on either side, which is wave-uniform.
__device__ void build_features(Side (&S)[2], const unsigned char* __restrict__ rec0, const unsigned char* __restrict__ rec1, int n0, int n1,
                               int drop_h, int R, int lane) {
  const int idx = lane & 31, side = lane >> 5;
  Side& me = S[side];
  const unsigned char* __restrict__ mine = side ? rec1 : rec0;
  const bool present = idx < (side ? n1 : n0);                               // n <= 29: lanes 29..31 of a half hold no atom
  const unsigned type = present ? mine[DS_REC_TYPE + idx] : 0u, fc = present ? mine[DS_REC_FC + idx] : 0u;
  const bool keep = present && !(drop_h && type == 0u);
  const unsigned long long kept_both = __ballot(keep);
  const unsigned kept = side ? (unsigned)(kept_both >> 32) : (unsigned)kept_both;
  const unsigned any = (unsigned)(kept_both >> 32) | (unsigned)kept_both;
  const unsigned hydrogens = drop_h ? half_ballot(present && type == 0u, side) : 0u;
  const int most = max(__popc((unsigned)kept_both), __popc((unsigned)(kept_both >> 32)));
  // bond bytes between the atoms below n (the dropped hydrogens are still counted in h_i)
  if (n0 > 0) ds_rec::load_bonds(S[0].adj, rec0, (1u << n0) - 1u, lane);
  if (n1 > 0) ds_rec::load_bonds(S[1].adj, rec1, (1u << n1) - 1u, lane);
  __syncthreads();
  const int row = min(idx, MA - 1) * 32;
  unsigned bonded = 0u;
  for (int j = 0; j < MA; ++j)
    if (keep && me.adj[row + j]) bonded |= 1u << j;
  const unsigned nb = bonded & kept;
  const unsigned d = (unsigned)__popc(nb), h = (unsigned)__popc(bonded & hydrogens);
  me.nb[idx] = nb;

  // c_i: for every atom i, the components of the kept graph without i
  unsigned cyc = 0u;
  for (unsigned todo = any; todo; todo &= todo - 1u) {                       // at most 29 atoms
    const int i = __ffs(todo) - 1;
    unsigned reach = (keep && idx != i) ? ((1u << idx) | nb) & ~(1u << i) : 0u;
    for (int s = 1; s < most; s <<= 1) {                                     // at most 5 squarings: paths of up to 2^5 bonds
      unsigned next = reach;
      for (unsigned rest = any; rest; rest &= rest - 1u) {
        const int k = __ffs(rest) - 1;
        const unsigned of_k = half_read(reach, k, side);
        if ((reach >> k) & 1u) next |= of_k;
      }
      reach = next;
    }
    const unsigned nb_i = half_read(nb, i, side);
    const unsigned two = half_ballot(((nb_i >> idx) & 1u) && (reach & nb_i & ~(1u << idx)), side);
    if (idx == i && two) cyc = 1u;
  }

  unsigned long long id = mix2(mix2(mix2(mix2(type, fc), d), h), cyc);
  me.feat[idx] = id;                                                         // layer 0
  me.ok[idx] = keep;
  me.id[idx] = id;
  __syncthreads();
  unsigned ball = keep ? 1u << idx : 0u;
  for (int r = 1; r <= R; ++r) {
    unsigned long long acc = 0ull;
    unsigned edge = 0u, canon = ball;
    for (unsigned rest = any; rest; rest &= rest - 1u) {
      const int k = __ffs(rest) - 1;
      const unsigned nb_k = me.nb[k];
      if ((nb >> k) & 1u) acc += mix2(me.id[k], me.adj[row + k]);
      if ((ball >> k) & 1u) edge |= nb_k;
      if (((kept >> k) & 1u) && !(nb_k & ~ball)) canon |= 1u << k;
    }
    const unsigned env = (keep && edge) ? canon : EMPTY;
    bool fresh = env != EMPTY;
    for (int s = 0; s < r - 1; ++s)
      for (unsigned rest = any; rest; rest &= rest - 1u) fresh = fresh && me.env[s][__ffs(rest) - 1] != env;
    id = mix2(mix2(id, (unsigned long long)r), acc);
    ball |= edge;
    __syncthreads();                                                         // every lane has read id_{r-1}
    me.id[idx] = id;
    me.env[r - 1][idx] = env;
    me.fresh[idx] = fresh;
    __syncthreads();
    // one value per distinct new bond set: its lowest atom holds the smallest id_r of the atoms that share it
    unsigned long long value = id;
    bool leader = fresh;
    for (unsigned rest = any; rest; rest &= rest - 1u) {
      const int k = __ffs(rest) - 1;
      if (me.fresh[k] && me.env[r - 1][k] == env) {
        const unsigned long long other = me.id[k];
        value = other < value ? other : value;
        if (k < idx) leader = false;
      }
    }
    me.feat[r * 32 + idx] = value;
    me.ok[r * 32 + idx] = leader;
  }
  __syncthreads();
}

// Marks in M.first the slots that count as elements of the set { f & mask }: a feature, and no lower slot holds the same value.  All 64 lanes
// work on the one side, two slots each.  Returns the size of the set.
__device__ int distinct(Side& M, int nslots, unsigned long long mask, int lane) {
  int total = 0;
  bool mine[SLOTS / 64];
#pragma unroll
  for (int half = 0; half < SLOTS / 64; ++half) {
    const int s = lane + 64 * half;
    bool own = s < nslots && M.ok[s];
    const unsigned long long v = own ? M.feat[s] & mask : 0ull;
    for (int t = 0; t < nslots; ++t)
      if (t < s && M.ok[t] && (M.feat[t] & mask) == v) own = false;
    mine[half] = own;
    total += __popcll(__ballot(own));
  }
#pragma unroll
  for (int half = 0; half < SLOTS / 64; ++half) M.first[lane + 64 * half] = mine[half];
  __syncthreads();
  return total;
}

__global__ __launch_bounds__(64) void k_morgan_records(const unsigned char* __restrict__ rec, const int32_t* __restrict__ n_atoms, int drop_h,
                                                       int R, unsigned long long* __restrict__ ids, int32_t* __restrict__ count) {
  __shared__ Side S[2];
  const int64_t p = blockIdx.x;
  const int lane = threadIdx.x;
  const unsigned char* __restrict__ mine = rec + p * DS_RECORD_BYTES;
  build_features(S, mine, mine, ds_rec::atoms_of(n_atoms, p), 0, drop_h, R, lane);       // the upper half holds no molecule
  const int nslots = (R + 1) * 32;
  const int total = distinct(S[0], nslots, ~0ull, lane);                     // <= 29 (R + 1) <= 116: only atoms' slots hold features
  unsigned long long* __restrict__ out = ids + p * DS_MORGAN_MAX_FEATURES;
#pragma unroll
  for (int half = 0; half < SLOTS / 64; ++half) {
    const int s = lane + 64 * half;
    const bool own = S[0].first[s];
    const unsigned long long v = own ? S[0].feat[s] : 0ull;
    int rank = 0;                                                            // distinct features below mine
    for (int t = 0; t < nslots; ++t) rank += S[0].first[t] && S[0].feat[t] < v;
    if (own && rank < DS_MORGAN_MAX_FEATURES) out[rank] = v;
  }
  for (int k = total + lane; k < DS_MORGAN_MAX_FEATURES; k += 64) out[k] = 0ull;
  if (lane == 0) count[p] = total;
}

__global__ __launch_bounds__(64) void k_morgan_similarity(const unsigned char* __restrict__ prb_rec, const int32_t* __restrict__ prb_n,
                                                          const unsigned char* __restrict__ ref_rec, const int32_t* __restrict__ ref_n,
                                                          const int64_t* __restrict__ ref_index, int64_t M, int drop_h, int R, int n_bits,
                                                          int32_t* __restrict__ common, int32_t* __restrict__ n_prb, int32_t* __restrict__ n_ref,
                                                          unsigned char* __restrict__ status) {
  __shared__ Side S[2];
  const int64_t p = blockIdx.x;
  const int lane = threadIdx.x;
  const ds_rec::Pair q = ds_rec::pair_of(p, prb_rec, prb_n, ref_rec, ref_n, ref_index, M);
  if (!q.valid) {
    if (lane == 0) { common[p] = -1; n_prb[p] = -1; n_ref[p] = -1; status[p] = DS_MORGAN_INVALID; }
    return;
  }
  build_features(S, q.prb, q.ref, q.n_prb(), q.n_ref(), drop_h, R, lane);
  const int nslots = (R + 1) * 32;
  const unsigned long long mask = n_bits ? (unsigned long long)(n_bits - 1) : ~0ull;     // n_bits is a power of two: f mod n_bits
  const int na = distinct(S[0], nslots, mask, lane), nb = distinct(S[1], nslots, mask, lane);
  int both = 0;
#pragma unroll
  for (int half = 0; half < SLOTS / 64; ++half) {
    const int s = lane + 64 * half;
    const bool own = S[0].first[s];
    const unsigned long long v = own ? S[0].feat[s] & mask : 0ull;
    bool hit = false;
    for (int t = 0; t < nslots; ++t) hit = hit || (S[1].first[t] && (S[1].feat[t] & mask) == v);
    both += __popcll(__ballot(own && hit));
  }
  if (lane == 0) { common[p] = both; n_prb[p] = na; n_ref[p] = nb; status[p] = DS_MORGAN_OK; }
}

inline bool shape_ok(int32_t drop_h, int32_t radius) { return (drop_h == 0 || drop_h == 1) && radius >= 0 && radius <= DS_MORGAN_MAX_RADIUS; }

}  // namespace

extern "C" int ds_morgan_records(const uint8_t* rec, const int32_t* n, int64_t P, int32_t drop_h, int32_t radius, uint64_t* ids, int32_t* count,
                                 void* stream) {
  const int go = ds_rec::check_table(shape_ok(drop_h, radius), P, rec, n, {ids, count});
  if (go != ds_rec::LAUNCH) return go;
  hipLaunchKernelGGL(k_morgan_records, dim3((unsigned)P), dim3(64), 0, (hipStream_t)stream, rec, n, (int)drop_h, (int)radius,
                     reinterpret_cast<unsigned long long*>(ids), count);
  return DST_CHECK_LAUNCH();
}

extern "C" int ds_morgan_similarity_records(const uint8_t* prb_rec, const int32_t* prb_n, int64_t P, const uint8_t* ref_rec, const int32_t* ref_n,
                                            int64_t M, const int64_t* ref_index, int32_t drop_h, int32_t radius, int32_t n_bits, int32_t* common,
                                            int32_t* n_prb, int32_t* n_ref, uint8_t* status, void* stream) {
  const bool fold_ok = n_bits == 0 || (n_bits >= 64 && n_bits <= DS_MORGAN_MAX_BITS && !(n_bits & (n_bits - 1)));
  const int go = ds_rec::check_pairs(shape_ok(drop_h, radius) && fold_ok, P, M, prb_rec, prb_n, ref_rec, ref_n, ref_index,
                                     {common, n_prb, n_ref, status});
  if (go != ds_rec::LAUNCH) return go;
  hipLaunchKernelGGL(k_morgan_similarity, dim3((unsigned)P), dim3(64), 0, (hipStream_t)stream, prb_rec, prb_n, ref_rec, ref_n, ref_index, M,
                     (int)drop_h, (int)radius, (int)n_bits, common, n_prb, n_ref, status);
  return DST_CHECK_LAUNCH();
}
