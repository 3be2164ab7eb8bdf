// diffspectra_amd - set-against-set analytics on packed Morgan bit rows: the fold of a feature list into a bit row and the all-pairs
// Tanimoto scan behind SNN and IntDiv.  include/diffspectra_sets.h states the definitions, the tie rule and the order of summation;
// DESIGN.md section 15 has the method and the figures.
//
// Three kernels, no atomics on global memory:
//   k_fold_bits        one wave per row: the bits are ORed into an LDS row (LDS atomics), the row's popcount is a wave sum;
//   k_tanimoto_pairs   grid (row tile, chunk), DSS_TILE_A threads, compiled per dword count W of a row: a lane keeps its A row in W registers,
//                      a tile of DSS_TILE_B rows of B sits in LDS and is read as 16-byte broadcasts (every lane reads the same address).  Per
//                      dword of a pair one v_and_b32 and one v_bcnt_u32_b32 that accumulates; per pair the integer comparison of the nearest
//                      neighbour (24-bit multiplies: c, u < 2^13) and one fp64 division.  Chunk g takes the column tiles g, g + K, ... and leaves
//                      (c, u, j, sum) per row in the workspace;
//   k_tanimoto_merge   one thread per A row merges the K partials in chunk order and writes the five outputs.
// Inside the kernels a similarity is the pair (c', u') = (c, u), or (1, 1) for u = 0: T = c' / u' with u' >= 1 always; "no row yet" is j = -1.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/diffspectra_sets.h"
#include "ds_host.h"   // DST_CHECK_LAUNCH

namespace {

constexpr int TILE_A = DSS_TILE_A, TILE_B = DSS_TILE_B, CHUNKS = DSS_CHUNKS, SLOTS = DS_MORGAN_MAX_FEATURES;
constexpr int64_t WS_PER_PARTIAL = sizeof(double) + 3 * sizeof(int32_t);      // sum, c', u', j of one (chunk, row)
static_assert(TILE_A % 64 == 0 && TILE_B <= TILE_A && TILE_B % 2 == 0, "whole waves; the popcounts of a tile are loaded by its first lanes");
static_assert(TILE_B * (DS_MORGAN_MAX_BITS / 8) + TILE_B * 4 <= 80 * 1024, "two workgroups share a CU's 160 KiB of LDS at every n_bits");

inline bool bits_ok(int32_t n_bits) { return n_bits >= 64 && n_bits <= DS_MORGAN_MAX_BITS && !(n_bits & (n_bits - 1)); }
inline int64_t chunks_of(int64_t Nb) {
  const int64_t tiles = (Nb + TILE_B - 1) / TILE_B;
  return tiles < 1 ? 1 : tiles < CHUNKS ? tiles : CHUNKS;
}

__global__ __launch_bounds__(64) void k_fold_bits(const unsigned long long* __restrict__ ids, const int32_t* __restrict__ count, int n_bits,
                                                  unsigned long long* __restrict__ words, int32_t* __restrict__ popcount) {
  __shared__ unsigned int row[DS_MORGAN_MAX_BITS / 32];
  const int64_t p = blockIdx.x;
  const int lane = threadIdx.x;
  const int nw = n_bits / 64;                                                  // <= 64: a word per lane
  row[lane] = 0u;
  row[lane + 64] = 0u;
  __syncthreads();
  int cnt = count[p];
  cnt = cnt < 0 ? 0 : cnt > SLOTS ? SLOTS : cnt;
  for (int k = lane; k < cnt; k += 64) {
    const unsigned int b = (unsigned int)(ids[p * SLOTS + k] & (unsigned long long)(n_bits - 1));
    atomicOr(&row[b >> 5], 1u << (b & 31));
  }
  __syncthreads();
  unsigned long long w = 0ull;
  if (lane < nw) {
    w = (unsigned long long)row[2 * lane] | ((unsigned long long)row[2 * lane + 1] << 32);
    words[p * nw + lane] = w;
  }
  int c = __popcll(w);
#pragma unroll
  for (int o = 32; o; o >>= 1) c += __shfl_xor(c, o);
  if (lane == 0) popcount[p] = c;
}

// popcount(x) + acc in one v_bcnt_u32_b32.  (Written as __popc(x) + acc the compiler re-associates a row's chain into counts against 0 and
// three-operand adds: one more instruction for every three dwords.)
__device__ __forceinline__ int bcnt_add(unsigned int x, int acc) {
  int out;
  asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(out) : "v"(x), "v"(acc));
  return out;
}

// a * b for 0 <= a, b < 2^13 (c' and u' are): the masks let the compiler take the full-rate 24-bit multiply
__device__ __forceinline__ int mul13(int a, int b) { return (a & 0x1fff) * (b & 0x1fff); }

// W dwords of row r, W >= 4 by 16 bytes, W = 2 by 8
template <int W>
__device__ __forceinline__ void load_row(const unsigned int* __restrict__ src, unsigned int (&a)[W]) {
  if constexpr (W >= 4) {
#pragma unroll
    for (int k = 0; k < W / 4; ++k) {
      const uint4 v = reinterpret_cast<const uint4*>(src)[k];
      a[4 * k] = v.x; a[4 * k + 1] = v.y; a[4 * k + 2] = v.z; a[4 * k + 3] = v.w;
    }
  } else {
    const uint2 v = *reinterpret_cast<const uint2*>(src);
    a[0] = v.x; a[1] = v.y;
  }
}

template <int W>
__global__ __launch_bounds__(TILE_A) void k_tanimoto_pairs(const unsigned int* __restrict__ a_words, const int32_t* __restrict__ a_pop, int64_t Na,
                                                           const unsigned int* __restrict__ b_words, const int32_t* __restrict__ b_pop, int64_t Nb,
                                                           int skip, double* __restrict__ ws_sum, int32_t* __restrict__ ws_c,
                                                           int32_t* __restrict__ ws_u, int32_t* __restrict__ ws_j) {
  __shared__ __attribute__((aligned(16))) unsigned int tile[TILE_B * W];
  __shared__ int pop[TILE_B];
  const int tid = threadIdx.x;
  const int g = blockIdx.y, K = gridDim.y;
  const int64_t r = (int64_t)blockIdx.x * TILE_A + tid;
  const bool held = r < Na;
  unsigned int a[W];
#pragma unroll
  for (int k = 0; k < W; ++k) a[k] = 0u;
  if (held) load_row<W>(a_words + r * W, a);
  const int pa = held ? a_pop[r] : 0;
  const int64_t own = skip ? r : -1;                                           // the column this row leaves out
  int best_c = 0, best_u = 1, best_j = -1;
  double sum = 0.0;
  const int64_t tiles = (Nb + TILE_B - 1) / TILE_B;
  for (int64_t t = g; t < tiles; t += K) {
    const int64_t j0 = t * TILE_B;
    const int width = Nb - j0 < TILE_B ? (int)(Nb - j0) : TILE_B;
    __syncthreads();
    {
      const uint2* __restrict__ src = reinterpret_cast<const uint2*>(b_words + j0 * W);
      uint2* dst = reinterpret_cast<uint2*>(tile);
      for (int k = tid; k < width * (W / 2); k += TILE_A) dst[k] = src[k];
      if (tid < width) pop[tid] = b_pop[j0 + tid];
    }
    __syncthreads();
    const int own_jj = own >= j0 && own < j0 + width ? (int)(own - j0) : -1;
    for (int jj = 0; jj < width; ++jj) {
      const unsigned int* __restrict__ b = tile + jj * W;
      int c0 = 0, c1 = 0;                                                      // two chains of the accumulating population count
      if constexpr (W >= 4) {
#pragma unroll
        for (int k = 0; k < W / 4; ++k) {
          const uint4 v = reinterpret_cast<const uint4*>(b)[k];
          c0 = bcnt_add(a[4 * k] & v.x, c0);
          c1 = bcnt_add(a[4 * k + 1] & v.y, c1);
          c0 = bcnt_add(a[4 * k + 2] & v.z, c0);
          c1 = bcnt_add(a[4 * k + 3] & v.w, c1);
        }
      } else {
        const uint2 v = *reinterpret_cast<const uint2*>(b);
        c0 = bcnt_add(a[0] & v.x, c0);
        c1 = bcnt_add(a[1] & v.y, c1);
      }
      const int c = c0 + c1, u = pa + pop[jj] - c;
      const int empty = u == 0;                                                // two empty rows: 1 / 1
      const int cq = c + empty, uq = u + empty;
      const bool take = jj != own_jj;
      const double q = (double)cq / (double)uq;
      sum += take ? q : 0.0;
      const bool better = take & ((best_j < 0) | (mul13(cq, best_u) > mul13(best_c, uq)));
      best_c = better ? cq : best_c;
      best_u = better ? uq : best_u;
      best_j = better ? (int)j0 + jj : best_j;
    }
  }
  if (held) {
    const int64_t at = (int64_t)g * Na + r;
    ws_sum[at] = sum; ws_c[at] = best_c; ws_u[at] = best_u; ws_j[at] = best_j;
  }
}

__global__ __launch_bounds__(256) void k_tanimoto_merge(const int32_t* __restrict__ a_pop, int64_t Na, int64_t Nb, int skip, int K,
                                                        const double* __restrict__ ws_sum, const int32_t* __restrict__ ws_c,
                                                        const int32_t* __restrict__ ws_u, const int32_t* __restrict__ ws_j,
                                                        int32_t* __restrict__ best_common, int32_t* __restrict__ best_union,
                                                        int64_t* __restrict__ best_index, double* __restrict__ sum, int64_t* __restrict__ compared) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= Na) return;
  int bc = 0, bu = 1, bj = -1;
  double s = 0.0;
  for (int g = 0; g < K; ++g) {                                                // K = 0 when there is no row of B
    const int64_t at = (int64_t)g * Na + r;
    const int c = ws_c[at], u = ws_u[at], j = ws_j[at];
    s += ws_sum[at];
    if (j < 0) continue;
    const int mine = c * bu, theirs = bc * u;                                  // below 2^26
    if (bj < 0 || mine > theirs || (mine == theirs && j < bj)) { bc = c; bu = u; bj = j; }
  }
  if (bj >= 0 && a_pop[r] == 0 && bc == 1) { bc = 0; bu = 0; }                 // (1, 1) with an empty A row stands for two empty rows
  best_common[r] = bj < 0 ? -1 : bc;
  best_union[r] = bj < 0 ? -1 : bu;
  best_index[r] = bj;
  sum[r] = s;
  compared[r] = Nb - ((skip && r < Nb) ? 1 : 0);
}

template <int W>
void launch_pairs(dim3 grid, hipStream_t st, const uint64_t* a_words, const int32_t* a_pop, int64_t Na, const uint64_t* b_words, const int32_t* b_pop,
                  int64_t Nb, int skip, double* ws_sum, int32_t* ws_c, int32_t* ws_u, int32_t* ws_j) {
  hipLaunchKernelGGL((k_tanimoto_pairs<W>), grid, dim3(TILE_A), 0, st, reinterpret_cast<const unsigned int*>(a_words), a_pop, Na,
                     reinterpret_cast<const unsigned int*>(b_words), b_pop, Nb, skip, ws_sum, ws_c, ws_u, ws_j);
}

}  // namespace

extern "C" int dss_fold_bits(const uint64_t* ids, const int32_t* count, int64_t P, int32_t n_bits, uint64_t* words, int32_t* popcount,
                             void* stream) {
  if (P < 0 || P > 0x7fffffffll || !bits_ok(n_bits)) return DS_ERR_ARG;
  if (P == 0) return DS_OK;
  if (!ids || !count || !words || !popcount) return DS_ERR_ARG;
  hipLaunchKernelGGL(k_fold_bits, dim3((unsigned)P), dim3(64), 0, (hipStream_t)stream, reinterpret_cast<const unsigned long long*>(ids), count,
                     (int)n_bits, reinterpret_cast<unsigned long long*>(words), popcount);
  return DST_CHECK_LAUNCH();
}

extern "C" int dss_tanimoto_nn_workspace_bytes(int64_t Na, int64_t Nb, int64_t* bytes) {
  if (Na < 0 || Na > 0x7fffffffll || Nb < 0 || Nb > 0x7fffffffll || !bytes) return DS_ERR_ARG;
  *bytes = chunks_of(Nb) * Na * WS_PER_PARTIAL;
  return DS_OK;
}

extern "C" int dss_tanimoto_nn(const uint64_t* a_words, const int32_t* a_pop, int64_t Na, const uint64_t* b_words, const int32_t* b_pop, int64_t Nb,
                               int32_t n_bits, int32_t skip_same_index, void* workspace, int64_t workspace_bytes, int32_t* best_common,
                               int32_t* best_union, int64_t* best_index, double* sum, int64_t* compared, void* stream) {
  if (Na < 0 || Na > 0x7fffffffll || Nb < 0 || Nb > 0x7fffffffll || !bits_ok(n_bits)) return DS_ERR_ARG;
  if (skip_same_index != 0 && skip_same_index != 1) return DS_ERR_ARG;
  if (Na == 0) return DS_OK;
  if (!a_words || !a_pop || !best_common || !best_union || !best_index || !sum || !compared) return DS_ERR_ARG;
  const uintptr_t row_align = n_bits >= 128 ? 15 : 7;                          // rows are read 16 bytes at a time, 8 at 64 bits
  if ((reinterpret_cast<uintptr_t>(a_words) | reinterpret_cast<uintptr_t>(b_words)) & row_align) return DS_ERR_ARG;
  const int64_t K = Nb > 0 ? chunks_of(Nb) : 0;
  if (Nb > 0 && (!b_words || !b_pop || !workspace || workspace_bytes < K * Na * WS_PER_PARTIAL || reinterpret_cast<uintptr_t>(workspace) & 7))
    return DS_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  double* ws_sum = static_cast<double*>(workspace);                            // [K][Na] each: the doubles first, so everything is aligned
  int32_t* ws_c = reinterpret_cast<int32_t*>(ws_sum + K * Na);
  int32_t* ws_u = ws_c + K * Na;
  int32_t* ws_j = ws_u + K * Na;
  if (K > 0) {
    const dim3 grid((unsigned)((Na + TILE_A - 1) / TILE_A), (unsigned)K);
    const int skip = (int)skip_same_index;
    switch (n_bits / 32) {
      case 2: launch_pairs<2>(grid, st, a_words, a_pop, Na, b_words, b_pop, Nb, skip, ws_sum, ws_c, ws_u, ws_j); break;
      case 4: launch_pairs<4>(grid, st, a_words, a_pop, Na, b_words, b_pop, Nb, skip, ws_sum, ws_c, ws_u, ws_j); break;
      case 8: launch_pairs<8>(grid, st, a_words, a_pop, Na, b_words, b_pop, Nb, skip, ws_sum, ws_c, ws_u, ws_j); break;
      case 16: launch_pairs<16>(grid, st, a_words, a_pop, Na, b_words, b_pop, Nb, skip, ws_sum, ws_c, ws_u, ws_j); break;
      case 32: launch_pairs<32>(grid, st, a_words, a_pop, Na, b_words, b_pop, Nb, skip, ws_sum, ws_c, ws_u, ws_j); break;
      case 64: launch_pairs<64>(grid, st, a_words, a_pop, Na, b_words, b_pop, Nb, skip, ws_sum, ws_c, ws_u, ws_j); break;
      default: launch_pairs<128>(grid, st, a_words, a_pop, Na, b_words, b_pop, Nb, skip, ws_sum, ws_c, ws_u, ws_j); break;
    }
  }
  hipLaunchKernelGGL(k_tanimoto_merge, dim3((unsigned)((Na + 255) / 256)), dim3(256), 0, st, a_pop, Na, Nb, (int)skip_same_index, (int)K, ws_sum,
                     ws_c, ws_u, ws_j, best_common, best_union, best_index, sum, compared);
  return DST_CHECK_LAUNCH();
}
