// gfx950 kernels + C-ABI of the generic GEMMs: ds_gemm (fp32 operands, row groups, fused epilogue; 64- and 128-row tiles) and
// ds_gemm_split (split-fp16 operands on the f16 matrix pipe: the per-step adaLN table).  See include/diffspectra_hip.h.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/diffspectra_hip.h"
#include "ds_device.h"
#include "ds_host.h"

namespace {

// The per-step adaLN table GEMM ada[M, N] = temb_silu[M, 1024] * W + bias on the f16 matrix pipe with split operands
// (ds_device.h).  A arrives pre-split from k_temb_finish (halves [M][2][K]); 64 x 128 output tile per workgroup, each wave 64
// rows x 32 columns (a weight fragment feeds 6 MFMAs; 128-row tiles spilled their staging registers), A chunks of 64 k
// double-buffered in LDS with the next chunk fetched into registers while the current one is multiplied.
__global__ __launch_bounds__(256) void k_gemm_ada(const _Float16* __restrict__ A, const float* __restrict__ Wh, const float* __restrict__ bias,
                                                  float* __restrict__ C, int ldc, int M, int K, int N) {
  ds_fp16_saturate();
  constexpr int T = 64, KC = 64, LDH = 2 * KC + 8, MT = T / 32;
  __shared__ __attribute__((aligned(16))) _Float16 X[2][T][LDH];
  const int tid = threadIdx.x, wave = tid >> 6;
  const int row0 = blockIdx.x * T;
  const int col0 = (blockIdx.y * 4 + wave) * 32;
  const bool active = col0 < N;
  const int nchunks = K / KC;
  // staging registers as four named values (an array here ended up in scratch memory)
  float4 st0, st1, st2, st3;
  const int srow = tid >> 4, spiece = tid & 15;               // thread's piece of rows srow, srow + 16, srow + 32, srow + 48
  const size_t scol = (size_t)(spiece >> 3) * K + (spiece & 7) * 8;
  auto fetch = [&](int kc) {
    const _Float16* base = A + scol + kc * KC;
    st0 = *reinterpret_cast<const float4*>(base + (size_t)min(row0 + srow, M - 1) * 2 * K);
    st1 = *reinterpret_cast<const float4*>(base + (size_t)min(row0 + srow + 16, M - 1) * 2 * K);
    st2 = *reinterpret_cast<const float4*>(base + (size_t)min(row0 + srow + 32, M - 1) * 2 * K);
    st3 = *reinterpret_cast<const float4*>(base + (size_t)min(row0 + srow + 48, M - 1) * 2 * K);
  };
  auto stash = [&](int buf) {   // planes are adjacent in a tile row: piece 0..7 plane 0, 8..15 plane 1
    *reinterpret_cast<float4*>(&X[buf][srow][spiece * 8]) = st0;
    *reinterpret_cast<float4*>(&X[buf][srow + 16][spiece * 8]) = st1;
    *reinterpret_cast<float4*>(&X[buf][srow + 32][spiece * 8]) = st2;
    *reinterpret_cast<float4*>(&X[buf][srow + 48][spiece * 8]) = st3;
  };
  f32x16 acc[MT], lo[MT];
  acc_zero<MT>(acc);
  acc_zero<MT>(lo);
  // weights: a chunk's four k-blocks sit in a register ring that is re-requested for the NEXT chunk as soon as this chunk's
  // MFMAs are issued - their L2 round trip flies under the A staging and the barrier (ds_device.h, wave_mma_h_deep)
  const WStreamH wsw = wstream_h(Wh, N, K, active ? col0 : 0);
  WRingH<4> ring;
  wring_h<4>(ring, wsw, 0);
  fetch(0);
  stash(0);
  __syncthreads();
  for (int kc = 0; kc < nchunks; ++kc) {
    const int cur = kc & 1;
    if (kc + 1 < nchunks) fetch(kc + 1);
    if (active) wave_mma_h_deep<MT, false, 4, 4>(&X[cur][0][0], KC, wsw, ring, kc * 4, acc, lo, kc * 4);
    if (kc + 1 < nchunks) { wring_h<4>(ring, wsw, kc * 4 + 4); stash(cur ^ 1); }
    __syncthreads();
  }
  if (!active) return;
  split_finish<MT>(acc, lo);
  const int lane = tid & 63, r = lane & 31, hh = lane >> 5, col = col0 + r;
  const float bcol = bias ? bias[col] : 0.0f;
  const unsigned long long pw = reinterpret_cast<unsigned long long>(C + (size_t)row0 * ldc + col0);
  const unsigned long long pu = (static_cast<unsigned long long>(__builtin_amdgcn_readfirstlane(static_cast<int>(pw >> 32))) << 32) |
                                static_cast<unsigned int>(__builtin_amdgcn_readfirstlane(static_cast<int>(pw)));
  const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<float*>(pu), 0, 0x7fffffff, 0x00020000);
  const int voff = (4 * hh * ldc + r) * 4, rowb = ldc * 4;
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = m * 32 + (i & 3) + 8 * (i >> 2);
      if (row0 + row + 4 * hh < M) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(acc[m][i] + bcol), rc, voff, row * rowb, 0);
    }
}

// ------------------------------------------------------------------------------------------------
// Generic GEMM (see header).  64x128 output tile per workgroup, A staged through LDS in K-chunks of 64.
// Row-group addressing lets A be an unfold view (SpecFormer patches), C a slice of a [B, L, D] token buffer and
// R a per-position table broadcast over molecules, without any host-side copy.
struct GemmArgs {
  const float* A; int64_t lda; int a_grp_rows; int64_t a_grp_stride;
  const float* Wp; const float* bias;
  float* C; int64_t ldc; int c_grp_rows; int64_t c_grp_stride;
  int M, K, N, Npad;
  const float* R; int64_t ldr; int r_grp_rows;
  const float* cs; const float* csh;
  int a_silu;
};

__device__ __forceinline__ size_t grp_off(int row, int64_t ld, int grp_rows, int64_t grp_stride) {
  if (grp_rows <= 0) return (size_t)row * ld;
  const int g = row / grp_rows;
  return (size_t)g * grp_stride + (size_t)(row - g * grp_rows) * ld;
}

template <int ACT>
__global__ __launch_bounds__(256) void k_gemm(GemmArgs g) {
  constexpr int T = 64, KC = 64;
  __shared__ __attribute__((aligned(16))) float X[T][KC + DS_LDP];
  __shared__ size_t arow[T];
  const int tid = threadIdx.x, wave = tid >> 6;
  const int row0 = blockIdx.x * T;
  const int col0 = (blockIdx.y * 4 + wave) * 32;
  const bool active = col0 < g.Npad;
  if (tid < T) arow[tid] = (row0 + tid < g.M) ? grp_off(row0 + tid, g.lda, g.a_grp_rows, g.a_grp_stride) : 0;
  f32x16 acc[2];
  acc_zero<2>(acc);
  const int Kpad = (g.K + 7) & ~7;
  for (int k0 = 0; k0 < Kpad; k0 += KC) {
    __syncthreads();
    for (int idx = tid; idx < T * KC; idx += 256) {
      const int row = idx >> 6, k = idx & 63;
      float v = 0.0f;
      if (row0 + row < g.M && k0 + k < g.K) {
        v = g.A[arow[row] + k0 + k];
        if (g.a_silu) v = ds_silu(v);
      }
      X[row][k] = v;
    }
    __syncthreads();
    if (active) {
      const int kgs = min(KC, Kpad - k0) >> 3;
      wave_mma<2>(&X[0][0], KC + DS_LDP, g.Wp + (size_t)(k0 >> 3) * 2 * g.Npad * 4, g.Npad, col0, 0, kgs, acc);
    }
  }
  if (!active) return;
  acc_foreach<2>(acc, 0, col0, [&](int row, int col, float v) {
    const int gr = row0 + row;
    if (gr < g.M && col < g.N) {
      if (g.bias) v += g.bias[col];
      v = ds_act<ACT>(v);
      if (g.R) v += g.R[(size_t)(g.r_grp_rows > 0 ? gr % g.r_grp_rows : gr) * g.ldr + col];
      if (g.cs) v = v * g.cs[col] + g.csh[col];
      g.C[grp_off(gr, g.ldc, g.c_grp_rows, g.c_grp_stride) + col] = v;
    }
  });
}

// Large plain GEMMs (the per-step adaLN table [B,1024] x [1024,19744] is 6 % of a denoising step): 128x128 output tile,
// MT = 4 (each B fragment feeds 16 MFMAs), A double-buffered in LDS with the next K-chunk fetched into registers while
// the current one is multiplied (one barrier per chunk), the next chunk's first B group requested ahead of that barrier.
// Requires contiguous rows (no row groups), K % 64 == 0 and 16-byte aligned rows.
template <int ACT>
__global__ __launch_bounds__(256, 2) void k_gemm_big(GemmArgs g) {
  constexpr int T = 128, KC = 64, LD = KC + DS_LDP;
  __shared__ __attribute__((aligned(16))) float X[2][T][LD];
  const int tid = threadIdx.x, wave = tid >> 6;
  const int row0 = blockIdx.x * T;
  const int col0 = (blockIdx.y * 4 + wave) * 32;
  const bool active = col0 < g.Npad;
  const int nchunks = g.K / KC;
  float4 st[8];
  auto fetch = [&](int kc) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int idx = tid + u * 256, row = idx >> 4, k4 = idx & 15;
      const size_t gr = (size_t)min(row0 + row, g.M - 1);
      st[u] = reinterpret_cast<const float4*>(g.A + gr * g.lda + (size_t)kc * KC)[k4];
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int idx = tid + u * 256, row = idx >> 4, k4 = idx & 15;
      float4 v = st[u];
      if (g.a_silu) { v.x = ds_silu(v.x); v.y = ds_silu(v.y); v.z = ds_silu(v.z); v.w = ds_silu(v.w); }
      if (row0 + row >= g.M) v = make_float4(0, 0, 0, 0);
      reinterpret_cast<float4*>(&X[buf][row][0])[k4] = v;
    }
  };
  f32x16 acc[4];
  acc_zero<4>(acc);
  fetch(0);
  stash(0);
  BFrag bf = bfrag_load(g.Wp, g.Npad, active ? col0 : 0, 0, 8);
  __syncthreads();
  for (int kc = 0; kc < nchunks; ++kc) {
    const int cur = kc & 1;
    if (kc + 1 < nchunks) fetch(kc + 1);
    const float* wp = g.Wp + (size_t)(kc * (KC / 8)) * 2 * g.Npad * 4;
    if (active) wave_mma<4>(&X[cur][0][0], LD, wp, g.Npad, col0, 0, KC / 8, acc, 0, &bf);
    if (kc + 1 < nchunks) {
      stash(cur ^ 1);
      bf = bfrag_load(wp + (size_t)(KC / 8) * 2 * g.Npad * 4, g.Npad, active ? col0 : 0, 0, 8);
    }
    __syncthreads();
  }
  if (!active) return;
  {   // epilogue: the lane's column constants are fetched once, rows go out as buffer stores with SGPR row offsets
    const int lane = tid & 63, r = lane & 31, hh = lane >> 5, col = col0 + r;
    const bool colok = col < g.N;
    const float bcol = (g.bias && colok) ? g.bias[col] : 0.0f;
    const float csc = (g.cs && colok) ? g.cs[col] : 1.0f, csh = (g.cs && colok) ? g.csh[col] : 0.0f;
    const unsigned long long pw = reinterpret_cast<unsigned long long>(g.C + (size_t)row0 * g.ldc + col0);
    const unsigned long long pu = (static_cast<unsigned long long>(__builtin_amdgcn_readfirstlane(static_cast<int>(pw >> 32))) << 32) |
                                  static_cast<unsigned int>(__builtin_amdgcn_readfirstlane(static_cast<int>(pw)));
    const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<float*>(pu), 0, 0x7fffffff, 0x00020000);
    const int voff = (4 * hh * g.ldc + r) * 4, rowb = g.ldc * 4;
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int row = m * 32 + (i & 3) + 8 * (i >> 2), gr = row0 + row + 4 * hh;
        if (gr < g.M && colok) {
          float v = ds_act<ACT>(acc[m][i] + bcol);
          if (g.R) v += g.R[(size_t)(g.r_grp_rows > 0 ? gr % g.r_grp_rows : gr) * g.ldr + col];
          if (g.cs) v = v * csc + csh;
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rc, voff, row * rowb, 0);
        }
      }
  }
}

// route_rows: the row count that picks the tile form (g.M, except for dst::gemm_routed_as).  A row's result does not depend on how
// many rows a launch has - both kernels clamp their loads to row M - 1 and guard their stores - but the two forms are not
// held to the same bits, so a caller that needs the bits of a larger launch's rows names that launch's size.
int gemm_dispatch(const GemmArgs& g, int act, hipStream_t s, int route_rows) {
  if (!g.A || !g.Wp || !g.C || g.M <= 0 || g.K <= 0 || g.N <= 0 || (g.cs && !g.csh)) return DS_ERR_ARG;
  const bool big = route_rows >= 512 && g.a_grp_rows <= 0 && g.c_grp_rows <= 0 && g.K % 64 == 0 && g.lda % 4 == 0 &&
                   (reinterpret_cast<uintptr_t>(g.A) & 15) == 0;
  using Kernel = void (*)(GemmArgs);   // one instantiation per activation code: 128-row tiles when big, else 64-row tiles
  static constexpr Kernel tile128[4] = {k_gemm_big<0>, k_gemm_big<1>, k_gemm_big<2>, k_gemm_big<3>};
  static constexpr Kernel tile64[4] = {k_gemm<0>, k_gemm<1>, k_gemm<2>, k_gemm<3>};
  if (act < 0 || act > 3) return DS_ERR_ARG;
  const int rows = big ? 128 : 64;
  hipLaunchKernelGGL(big ? tile128[act] : tile64[act], dim3((g.M + rows - 1) / rows, (g.Npad + 127) / 128), dim3(256), 0, s, g);
  return DST_CHECK_LAUNCH();
}

GemmArgs gemm_args(const ds_gemm_args* a) {
  GemmArgs g{};
  g.A = a->A; g.lda = a->lda; g.a_grp_rows = a->a_grp_rows; g.a_grp_stride = a->a_grp_stride;
  g.Wp = a->Wp; g.bias = a->bias;
  g.C = a->C; g.ldc = a->ldc; g.c_grp_rows = a->c_grp_rows; g.c_grp_stride = a->c_grp_stride;
  g.M = a->M; g.K = a->K; g.N = a->N; g.Npad = (a->N + 31) & ~31;
  g.R = a->R; g.ldr = a->ldr; g.r_grp_rows = a->r_grp_rows;
  g.cs = a->col_scale; g.csh = a->col_shift; g.a_silu = a->a_silu;
  return g;
}

}  // namespace

int dst::gemm_routed_as(const ds_gemm_args* a, int route_rows, void* stream) {
  if (!a || route_rows < a->M) return DS_ERR_ARG;
  return gemm_dispatch(gemm_args(a), a->act, (hipStream_t)stream, route_rows);
}

extern "C" {

int ds_gemm(const ds_gemm_args* a, void* stream) {
  if (!a) return DS_ERR_ARG;
  return gemm_dispatch(gemm_args(a), a->act, (hipStream_t)stream, a->M);
}

int ds_gemm_split(const void* A_split, const float* W_split, const float* bias, float* C, int64_t ldc, int32_t M, int32_t K,
                  int32_t N, void* stream) {
  if (!A_split || !W_split || !C || M <= 0 || K <= 0 || N <= 0 || K % 64 != 0 || N % 32 != 0 || ldc < N) return DS_ERR_ARG;
  hipLaunchKernelGGL(k_gemm_ada, dim3((M + 63) / 64, (N + 127) / 128), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const _Float16*>(A_split), W_split, bias, C, (int)ldc, M, K, N);
  return DST_CHECK_LAUNCH();
}

}  // extern "C"
