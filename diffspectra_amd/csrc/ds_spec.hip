// gfx950 kernels + C-ABI of SpecFormer inference: the residual-score attention and the affine LayerNorm.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/diffspectra_hip.h"
#include "ds_device.h"
#include "ds_host.h"

namespace {

// SpecFormer residual-score attention (specformer.py:401-424): one workgroup per (molecule, head) and up to 1024 queries - one
// query per thread, K / V of the head staged in LDS once for all of them.
// qkv [B, L, 3*heads*dk] (q | k | v); scores [B, heads, L, L] holds prev on entry (if has_prev) and the new
// pre-softmax scores on exit; out [B, L, heads*dk].
__global__ __launch_bounds__(1024) void k_spec_attention(const float* __restrict__ qkv, float* __restrict__ scores,
                                                       float* __restrict__ out, int B, int L, int heads, float scale,
                                                       int has_prev) {
  constexpr int DK = 8;
  extern __shared__ __attribute__((aligned(16))) float kv[];   // K [L][8] then V [L][8]
  const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * blockDim.x, tid = threadIdx.x;
  const int D = heads * DK;
  float* Ks = kv;
  float* Vs = kv + (size_t)L * DK;
  for (int idx = tid; idx < L * DK; idx += blockDim.x) {
    const int j = idx / DK, d = idx - j * DK;
    const float* base = qkv + ((size_t)b * L + j) * 3 * D + h * DK + d;
    Ks[idx] = base[D];
    Vs[idx] = base[2 * D];
  }
  __syncthreads();
  const int i = q0 + tid;
  if (i >= L) return;
  float q[DK];
  for (int d = 0; d < DK; ++d) q[d] = qkv[((size_t)b * L + i) * 3 * D + h * DK + d];
  // residual scores are kept TRANSPOSED, [b][h][key j][query i]: the lanes of a wave are consecutive queries, so every
  // access below is one contiguous 256-byte segment (query-major rows made each lane touch its own cache line)
  float* scol = scores + ((size_t)b * heads + h) * L * L + i;
  // One pass with a running maximum (the scores are written for the next layer and never read back here: the [B, heads, L, L]
  // tensor is this kernel's whole HBM bill - 4.1 GB per launch with the two-pass form).  Blocks of 8 keys: one rescale per block.
  float mx = -INFINITY, den = 0.0f, o[DK];
  for (int d = 0; d < DK; ++d) o[d] = 0.0f;
  for (int j0 = 0; j0 < L; j0 += 8) {
    float sv[8];
    float bm = -INFINITY;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int j = min(j0 + u, L - 1);
      float s = 0.0f;
#pragma unroll
      for (int d = 0; d < DK; ++d) s += q[d] * Ks[j * DK + d];
      s *= scale;
      if (has_prev) s += scol[(size_t)j * L];
      sv[u] = s;
      if (j0 + u < L) { scol[(size_t)j * L] = s; bm = fmaxf(bm, s); }
    }
    const float nm = fmaxf(mx, bm), r = expf(mx - nm);   // mx = -inf on the first block: r = 0
    den *= r;
#pragma unroll
    for (int d = 0; d < DK; ++d) o[d] *= r;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (j0 + u < L) {
        const float p = expf(sv[u] - nm);
        den += p;
#pragma unroll
        for (int d = 0; d < DK; ++d) o[d] += p * Vs[(j0 + u) * DK + d];
      }
    }
    mx = nm;
  }
  for (int d = 0; d < DK; ++d) out[((size_t)b * L + i) * D + h * DK + d] = o[d] / den;
}

__global__ void k_layernorm_affine(const float* __restrict__ x, const float* __restrict__ g, const float* __restrict__ bt,
                                   float* __restrict__ y, int rows, int cols, float eps) {
  const int row = blockIdx.x, lane = threadIdx.x;   // one wave per row
  if (row >= rows) return;
  const float* xr = x + (size_t)row * cols;
  float s = 0.0f;
  for (int k = lane; k < cols; k += 64) s += xr[k];
  const float mean = wave_sum(s) / (float)cols;
  float v = 0.0f;
  for (int k = lane; k < cols; k += 64) { const float d = xr[k] - mean; v += d * d; }
  const float rstd = 1.0f / sqrtf(wave_sum(v) / (float)cols + eps);
  for (int k = lane; k < cols; k += 64) y[(size_t)row * cols + k] = (xr[k] - mean) * rstd * g[k] + bt[k];
}

}  // namespace

extern "C" {

int ds_spec_attention(const float* qkv, float* scores, float* out, int B, int L, int heads, int dk, float scale, int has_prev,
                      void* stream) {
  if (!qkv || !scores || !out || dk != 8 || B <= 0 || L <= 0) return DS_ERR_ARG;
  const int threads = min(1024, (L + 63) / 64 * 64);
  dim3 grid((L + threads - 1) / threads, heads, B);
  hipLaunchKernelGGL(k_spec_attention, grid, dim3(threads), (size_t)L * 8 * 2 * sizeof(float), (hipStream_t)stream, qkv, scores, out, B,
                     L, heads, scale, has_prev);
  return DST_CHECK_LAUNCH();
}

int ds_layernorm_affine(const float* x, const float* gamma, const float* beta, float* y, int rows, int cols, float eps,
                        void* stream) {
  if (!x || !gamma || !beta || !y || rows <= 0 || cols <= 0) return DS_ERR_ARG;
  hipLaunchKernelGGL(k_layernorm_affine, dim3(rows), dim3(64), 0, (hipStream_t)stream, x, gamma, beta, y, rows, cols, eps);
  return DST_CHECK_LAUNCH();
}

}  // extern "C"
