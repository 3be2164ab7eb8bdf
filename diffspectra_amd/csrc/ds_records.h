// diffspectra_amd - what the per-pair evaluation kernels on result records share (ds_match.hip, ds_graph.hip, ds_mces.hip, ds_morgan.hip): the
// pair prologue, the bond-matrix loader, the 64-bit mix of the hashes and the host-side argument check of the "record pairs" contract in
// include/diffspectra_hip.h.  The record layout itself is the header's (DS_REC_*).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <initializer_list>

#include "../../include/diffspectra_hip.h"

namespace ds_rec {

constexpr int MA = DS_MAX_ATOMS;          // 29 atoms: an atom per lane, one molecule per half wave or per wave

// the value of lane 0 in every lane, as a wave-uniform (scalar) value
__device__ __forceinline__ int uniform_i(int v) { return __builtin_amdgcn_readfirstlane(v); }

// atoms of the molecule in row `row`, clamped to 0..29
__device__ __forceinline__ int atoms_of(const int32_t* __restrict__ n, int64_t row) { return min(max(n[row], 0), MA); }

// Pair p of a launch: its ground-truth row and both records.  A row outside ref_rec is an invalid pair, never a read: with `valid` false
// neither the records nor the counts may be touched (the counts are loaded on request, so that the loads stay behind the caller's branch).
struct Pair {
  int64_t p, r;
  const unsigned char *prb, *ref;
  const int32_t *prb_n, *ref_n;
  bool valid;
  __device__ __forceinline__ int n_prb() const { return atoms_of(prb_n, p); }
  __device__ __forceinline__ int n_ref() const { return atoms_of(ref_n, r); }
};

__device__ __forceinline__ Pair pair_of(int64_t p, const unsigned char* __restrict__ prb_rec, const int32_t* __restrict__ prb_n,
                                        const unsigned char* __restrict__ ref_rec, const int32_t* __restrict__ ref_n,
                                        const int64_t* __restrict__ ref_index, int64_t M) {
  const int64_t r = ref_index ? ref_index[p] : p;
  return {p, r, prb_rec + p * DS_RECORD_BYTES, ref_rec + r * DS_RECORD_BYTES, prb_n, ref_n, r >= 0 && r < M};
}

// Bond bytes of one record as a symmetric matrix adj[i * 32 + j] over original atom indices: the upper triangle of the record decides, the
// diagonal is no atom pair and reads 0, and a pair with an end outside `keep` (bit i = atom i is kept) reads 0, so all 29 x 29 entries are
// defined.  The record is read as aligned dwords; every byte index stays inside the record (static_assert in the header).  Inlined, so that
// an all-ones `keep` folds away.
__device__ __forceinline__ void load_bonds(unsigned char* __restrict__ adj, const unsigned char* __restrict__ rec, unsigned keep, int lane) {
  const uint32_t* __restrict__ words = reinterpret_cast<const uint32_t*>(rec);
  for (int w = DS_REC_BOND / 4 + lane; w < (DS_REC_BOND_END + 3) / 4; w += 64) {      // dwords 101 .. 311 of 312
    const uint32_t v = words[w];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = w * 4 + q - DS_REC_BOND;
      if (k < 0 || k >= MA * MA) continue;
      const int i = k / MA, j = k - i * MA;
      const unsigned char b = ((keep >> i) & (keep >> j) & 1u) ? (unsigned char)(v >> (8 * q)) : (unsigned char)0;
      if (i < j) { adj[i * 32 + j] = b; adj[j * 32 + i] = b; }
      else if (i == j) adj[i * 32 + i] = 0;
    }
  }
}

// the 64-bit finaliser and the pair mix of the header's hash formulas (ds_graph_hash_records, ds_morgan_records; wrap-around arithmetic)
__device__ __forceinline__ uint64_t fmix(uint64_t x) {
  x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27; x *= 0x94d049bb133111ebull;
  return x ^ (x >> 31);
}
__device__ __forceinline__ uint64_t mix2(uint64_t a, uint64_t b) { return fmix(a + 0x9e3779b97f4a7c15ull * (b + 1ull)); }

// Host side: the argument check of an entry point on one record table (ds_graph_hash_records, ds_morgan_records) and on record pairs, in the order the header
// states - `scalars_ok` (the entry point's own scalar arguments) and the sizes first, then P = 0, then the pointers.  Returns LAUNCH, or the
// status to return at once: DS_ERR_ARG, or DS_OK when there is nothing to do.
constexpr int LAUNCH = 1;

inline int check_table(bool scalars_ok, int64_t P, const void* rec, const void* n, std::initializer_list<const void*> outputs) {
  if (!scalars_ok || P < 0 || P > 0x7fffffffll) return DS_ERR_ARG;
  if (P == 0) return DS_OK;
  if (!rec || !n || reinterpret_cast<uintptr_t>(rec) & 3) return DS_ERR_ARG;          // records are read as dwords and hold fp32 positions
  for (const void* o : outputs)
    if (!o) return DS_ERR_ARG;
  return LAUNCH;
}

inline int check_pairs(bool scalars_ok, int64_t P, int64_t M, const void* prb_rec, const void* prb_n, const void* ref_rec, const void* ref_n,
                       const void* ref_index, std::initializer_list<const void*> outputs) {
  const int go = check_table(scalars_ok && M >= 0, P, prb_rec, prb_n, outputs);
  if (go != LAUNCH) return go;
  if (M > 0 && (!ref_rec || !ref_n)) return DS_ERR_ARG;
  if (!ref_index && M < P) return DS_ERR_ARG;                // identity pairing needs a ground-truth row for every pair
  return reinterpret_cast<uintptr_t>(ref_rec) & 3 ? DS_ERR_ARG : LAUNCH;
}

}  // namespace ds_rec
