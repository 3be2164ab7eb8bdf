// gfx950 kernels + C-ABI of the sampler side, which needs only a ds_layout: the ancestral update with host or in-kernel
// (Philox4x32-10 + Box-Muller) noise, the graph-replayable step counter, the multistep solver update (DDIM, DPM-Solver++(2M) ODE / SDE),
// post-processing and the stability check.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/diffspectra_hip.h"
#include "../../include/diffspectra_solver.h"
#include "ds_bonds.h"
#include "ds_host.h"

namespace {

using dst::clear;
using dst::layout_ok;

// the float2 operands of k_solver_step; NULL passes (whether a pointer may be NULL is each entry point's check)
bool edge_aligned8(std::initializer_list<const void*> ptrs) {
  for (const void* p : ptrs)
    if (reinterpret_cast<uintptr_t>(p) & 7) return false;
  return true;
}

// ------------------------------------------------------------------------------------------------
// Ancestral update, one workgroup per molecule (sampling.py:604-624; models/utils.py:38-45,67-106).
__global__ __launch_bounds__(256) void k_sampler_step(ds_layout L, float c_x, float c_pred, float sigma, float temp,
                                                      float* __restrict__ x, float* __restrict__ edge_x,
                                                      const float* __restrict__ pred, const float* __restrict__ edge_pred,
                                                      const float* __restrict__ raw_pos, const float* __restrict__ raw_feat,
                                                      const float* __restrict__ raw_edge, float* __restrict__ x_mean,
                                                      float* __restrict__ edge_mean) {
  __shared__ __attribute__((aligned(16))) float mean[3];
  __shared__ int dn[32];
  const int m = blockIdx.x, tid = threadIdx.x;
  const int n0 = L.node_off[m], n = L.node_off[m + 1] - n0;
  if (n <= 0) return;
  if (tid < n) dn[tid] = L.node_dense[n0 + tid];
  __syncthreads();
  if (tid < 3) {
    float s = 0.0f;
    for (int a = 0; a < n; ++a) s += raw_pos[(size_t)dn[a] * 3 + tid];
    mean[tid] = s / (float)n;
  }
  __syncthreads();
  for (int idx = tid; idx < n * 9; idx += 256) {
    const int a = idx / 9, ch = idx - a * 9;
    const size_t d = (size_t)dn[a];
    const float nz = ch < 3 ? raw_pos[d * 3 + ch] - mean[ch] : raw_feat[d * 6 + (ch - 3)];
    const float xm = c_x * x[d * 9 + ch] + c_pred * pred[d * 9 + ch];
    x_mean[d * 9 + ch] = xm;
    x[d * 9 + ch] = xm + (sigma * nz) * temp;
  }
  const int N = L.N;
  for (int idx = tid; idx < n * n * 2; idx += 256) {
    const int ch = idx & 1, ij = idx >> 1;
    const int a = ij / n, b = ij - a * n;
    if (a == b) continue;
    const int la = dn[a] - m * N, lb = dn[b] - m * N;
    const int hi = la > lb ? la : lb, lo = la > lb ? lb : la;
    const float nz = raw_edge[(((size_t)m * 2 + ch) * N + hi) * N + lo];   // tril(-1) + transpose
    const size_t o = ((size_t)dn[a] * N + lb) * 2 + ch;
    const float em = c_x * edge_x[o] + c_pred * edge_pred[o];
    edge_mean[o] = em;
    edge_x[o] = em + (sigma * nz) * temp;
  }
}

// ---- in-kernel noise: Philox4x32-10 (Salmon et al., SC'11; the generator torch/curand use) + Box-Muller ----
struct Philox4 { unsigned int x, y, z, w; };
__device__ __forceinline__ Philox4 philox4x32_10(unsigned int c0, unsigned int c1, unsigned int c2, unsigned int c3,
                                                 unsigned int k0, unsigned int k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned int hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned int hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const unsigned int n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return Philox4{c0, c1, c2, c3};
}
// u = (x + 0.5) / 2^32 in (0, 1]; (z0, z1) = sqrt(-2 ln u0) * (cos, sin)(2 pi u1)
__device__ __forceinline__ float2 box_muller(unsigned int a, unsigned int b) {
  const float u0 = __fmaf_rn((float)a, 2.3283064365386963e-10f, 1.1641532182693481e-10f);
  const float u1 = __fmaf_rn((float)b, 2.3283064365386963e-10f, 1.1641532182693481e-10f);
  const float r = sqrtf(-2.0f * logf(u0));
  const float th = 6.283185307179586f * u1;
  return make_float2(r * cosf(th), r * sinf(th));
}
__device__ __forceinline__ float4 philox_normal4(unsigned int elem, unsigned int draw, unsigned long long mol, unsigned int kind,
                                                 unsigned long long seed) {
  // counter words: (element, draw, mol_id low 32 bits, kind | mol_id high bits << 1)
  const Philox4 p = philox4x32_10(elem, draw, (unsigned int)mol, kind | ((unsigned int)(mol >> 32) << 1),
                                  (unsigned int)seed, (unsigned int)(seed >> 32));
  const float2 a = box_muller(p.x, p.y), b = box_muller(p.z, p.w);
  return make_float4(a.x, a.y, b.x, b.y);
}

// One workgroup per molecule.  MODE 0: initial noise (x, edge_x := noise; masked entries were zeroed by the caller's
// memset).  MODE 1: ancestral update with in-kernel noise (the Philox twin of k_sampler_step).
// MODE 2: as MODE 1 with (c_x, c_pred, sigma) and the draw index read from device memory (graph replay).
template <int MODE>
__global__ __launch_bounds__(256) void k_noise_step(ds_layout L, float c_x, float c_pred, float sigma, float temp,
                                                    unsigned long long seed, unsigned int draw, const int64_t* __restrict__ mol_id,
                                                    float* __restrict__ x, float* __restrict__ edge_x,
                                                    const float* __restrict__ pred, const float* __restrict__ edge_pred,
                                                    float* __restrict__ x_mean, float* __restrict__ edge_mean,
                                                    const float* __restrict__ table, const int32_t* __restrict__ step) {
  __shared__ __attribute__((aligned(16))) float nz[32][12];
  __shared__ float mean[3];
  __shared__ int dn[32];
  const int m = blockIdx.x, tid = threadIdx.x;
  const int n0 = L.node_off[m], n = L.node_off[m + 1] - n0;
  if (n <= 0) return;
  if (MODE == 2) {
    const int i = *step;
    c_x = table[4 * i]; c_pred = table[4 * i + 1]; sigma = table[4 * i + 2];
    draw = (unsigned int)i + 1u;
  }
  const unsigned long long mol = (unsigned long long)mol_id[m];
  if (tid < n) dn[tid] = L.node_dense[n0 + tid];
  if (tid < n * 3) {
    const int a = tid / 3, j = tid - a * 3;
    const float4 v = philox_normal4((unsigned int)tid, draw, mol, 0u, seed);
    reinterpret_cast<float4*>(&nz[a][4 * j])[0] = v;
  }
  __syncthreads();
  if (tid < 3) {   // CoM projection of the position noise (models/utils.py:38-45,88-93), atoms in ascending order
    float s = 0.0f;
    for (int a = 0; a < n; ++a) s += nz[a][tid];
    mean[tid] = s / (float)n;
  }
  __syncthreads();
  for (int idx = tid; idx < n * 9; idx += 256) {
    const int a = idx / 9, ch = idx - a * 9;
    const size_t d = (size_t)dn[a];
    const float v = ch < 3 ? nz[a][ch] - mean[ch] : nz[a][ch];
    if (MODE == 0) {
      x[d * 9 + ch] = v;
    } else {   // MODE 1, 2
      const float xm = c_x * x[d * 9 + ch] + c_pred * pred[d * 9 + ch];
      x_mean[d * 9 + ch] = xm;
      x[d * 9 + ch] = xm + (sigma * v) * temp;
    }
  }
  const int N = L.N, P = n * (n - 1) / 2;
  for (int p = tid; p < P; p += 256) {   // unordered pair lo < hi: p = hi(hi-1)/2 + lo, independent of n and of padding
    int hi = (int)((1.0f + sqrtf(1.0f + 8.0f * (float)p)) * 0.5f);
    while (hi * (hi - 1) / 2 > p) --hi;
    while ((hi + 1) * hi / 2 <= p) ++hi;
    const int lo = p - hi * (hi - 1) / 2;
    const float4 v = philox_normal4((unsigned int)p, draw, mol, 1u, seed);
    const int la = dn[lo] - m * N, lb = dn[hi] - m * N;
    const size_t o1 = ((size_t)dn[lo] * N + lb) * 2, o2 = ((size_t)dn[hi] * N + la) * 2;
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
      const float nzv = ch ? v.y : v.x;
      if (MODE == 0) {
        edge_x[o1 + ch] = nzv; edge_x[o2 + ch] = nzv;
      } else {
        const float em1 = c_x * edge_x[o1 + ch] + c_pred * edge_pred[o1 + ch];
        const float em2 = c_x * edge_x[o2 + ch] + c_pred * edge_pred[o2 + ch];
        edge_mean[o1 + ch] = em1; edge_mean[o2 + ch] = em2;
        edge_x[o1 + ch] = em1 + (sigma * nzv) * temp; edge_x[o2 + ch] = em2 + (sigma * nzv) * temp;
      }
    }
  }
}

// Opens a graph-replayable denoise iteration: ++*step, noise_level[b] = table[*step][3] (one workgroup).
__global__ __launch_bounds__(256) void k_step_begin(const float* __restrict__ table, int n_steps, int32_t* __restrict__ step, int B,
                                                    float* __restrict__ noise_level) {
  __shared__ int cur;
  if (threadIdx.x == 0) {
    const int i = min(*step + 1, n_steps - 1);
    *step = i;
    cur = i;
  }
  __syncthreads();
  const float nl = table[4 * cur + 3];
  for (int b = threadIdx.x; b < B; b += 256) noise_level[b] = nl;
}

// ------------------------------------------------------------------------------------------------
// Multistep solver update (include/diffspectra_solver.h): x_mean = ca x + cb pred + cc hist, x = x_mean + (cd noise) temp, in the frame of
// k_noise_step: one workgroup per molecule, the same Philox counters, CoM projection and pair order.  MODE 0: noise from raw_pos /
// raw_feat / raw_edge (the host twin, k_sampler_step's draws); MODE 1: in-kernel Philox; MODE 2: as MODE 1 with the row and the draw index
// read from device memory, and hist := pred once the old hist is read (graph replay).  cc == 0 and cd == 0 are uniform over the grid:
// the history is then not read, the noise neither generated nor loaded.  The two edge channels move as one float2.  Every sum is a
// spelled-out fma: left to the compiler, the contraction differed between (i,j) and (j,i) of one pair and symmetric input gave edges that
// differed in the last bit.
template <int MODE>
__global__ __launch_bounds__(256) void k_solver_step(ds_layout L, float ca, float cb, float cc, float cd, float temp,
                                                     unsigned long long seed, unsigned int draw, const int64_t* __restrict__ mol_id,
                                                     float* __restrict__ x, float* __restrict__ edge_x, const float* __restrict__ pred,
                                                     const float* __restrict__ edge_pred, float* __restrict__ hist,
                                                     float* __restrict__ edge_hist, const float* __restrict__ raw_pos,
                                                     const float* __restrict__ raw_feat, const float* __restrict__ raw_edge,
                                                     float* __restrict__ x_mean, float* __restrict__ edge_mean,
                                                     const float* __restrict__ table, const int32_t* __restrict__ step) {
  __shared__ __attribute__((aligned(16))) float nz[32][12];
  __shared__ float mean[3];
  __shared__ int dn[32];
  const int m = blockIdx.x, tid = threadIdx.x;
  const int n0 = L.node_off[m], n = L.node_off[m + 1] - n0;
  if (n <= 0) return;
  if (MODE == 2) {
    const int i = *step;
    const float* row = table + (size_t)DS_SOLVER_ROW * i;
    ca = row[0]; cb = row[1]; cc = row[2]; cd = row[3];
    draw = (unsigned int)i + 1u;
  }
  const bool use_hist = cc != 0.0f, use_noise = cd != 0.0f;
  if (tid < n) dn[tid] = L.node_dense[n0 + tid];
  unsigned long long mol = 0;
  if (use_noise) {
    if (MODE == 0) {
      __syncthreads();
      for (int idx = tid; idx < n * 9; idx += 256) {
        const int a = idx / 9, ch = idx - a * 9;
        const size_t g = (size_t)dn[a];
        nz[a][ch] = ch < 3 ? raw_pos[g * 3 + ch] : raw_feat[g * 6 + (ch - 3)];
      }
    } else {
      mol = (unsigned long long)mol_id[m];
      if (tid < n * 3) {
        const int a = tid / 3, j = tid - a * 3;
        const float4 v = philox_normal4((unsigned int)tid, draw, mol, 0u, seed);
        reinterpret_cast<float4*>(&nz[a][4 * j])[0] = v;
      }
    }
    __syncthreads();
    if (tid < 3) {   // CoM projection of the position noise, atoms in ascending order (as k_sampler_step / k_noise_step)
      float s = 0.0f;
      for (int a = 0; a < n; ++a) s += nz[a][tid];
      mean[tid] = s / (float)n;
    }
  }
  __syncthreads();
  for (int idx = tid; idx < n * 9; idx += 256) {
    const int a = idx / 9, ch = idx - a * 9;
    const size_t e = (size_t)dn[a] * 9 + ch;
    const float p = pred[e];
    float xm = __fmaf_rn(ca, x[e], cb * p);
    if (use_hist) xm = __fmaf_rn(cc, hist[e], xm);
    if (MODE == 2) hist[e] = p;
    x_mean[e] = xm;
    float xn = xm;
    if (use_noise) {
      const float v = ch < 3 ? nz[a][ch] - mean[ch] : nz[a][ch];
      xn = __fmaf_rn(cd * v, temp, xm);
    }
    x[e] = xn;
  }
  const int N = L.N, P = n * (n - 1) / 2;
  float2* __restrict__ ex2 = reinterpret_cast<float2*>(edge_x);
  float2* __restrict__ em2 = reinterpret_cast<float2*>(edge_mean);
  float2* __restrict__ eh2 = reinterpret_cast<float2*>(edge_hist);
  const float2* __restrict__ ep2 = reinterpret_cast<const float2*>(edge_pred);
  for (int p = tid; p < P; p += 256) {   // unordered pair lo < hi: p = hi(hi-1)/2 + lo, as k_noise_step
    int hi = (int)((1.0f + sqrtf(1.0f + 8.0f * (float)p)) * 0.5f);
    while (hi * (hi - 1) / 2 > p) --hi;
    while ((hi + 1) * hi / 2 <= p) ++hi;
    const int lo = p - hi * (hi - 1) / 2;
    const int la = dn[lo] - m * N, lb = dn[hi] - m * N;
    float2 nv = make_float2(0.0f, 0.0f);
    if (use_noise) {
      if (MODE == 0) {   // tril(-1) + transpose of raw_edge [B,2,N,N]
        const int r = la > lb ? la : lb, q = la > lb ? lb : la;
        nv.x = raw_edge[(((size_t)m * 2 + 0) * N + r) * N + q];
        nv.y = raw_edge[(((size_t)m * 2 + 1) * N + r) * N + q];
      } else {
        const float4 v = philox_normal4((unsigned int)p, draw, mol, 1u, seed);
        nv.x = v.x; nv.y = v.y;
      }
    }
    const size_t o[2] = {(size_t)dn[lo] * N + lb, (size_t)dn[hi] * N + la};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const float2 xv = ex2[o[s]], pv = ep2[o[s]];
      float2 em = make_float2(__fmaf_rn(ca, xv.x, cb * pv.x), __fmaf_rn(ca, xv.y, cb * pv.y));
      if (use_hist) {
        const float2 hv = eh2[o[s]];
        em.x = __fmaf_rn(cc, hv.x, em.x); em.y = __fmaf_rn(cc, hv.y, em.y);
      }
      if (MODE == 2) eh2[o[s]] = pv;
      em2[o[s]] = em;
      ex2[o[s]] = use_noise ? make_float2(__fmaf_rn(cd * nv.x, temp, em.x), __fmaf_rn(cd * nv.y, temp, em.y)) : em;
    }
  }
}

// k_step_begin for the solver's 32-byte rows: ++*step, noise_level[b] = table[*step][4] (one workgroup).
__global__ __launch_bounds__(256) void k_solver_step_begin(const float* __restrict__ table, int n_steps, int32_t* __restrict__ step, int B,
                                                           float* __restrict__ noise_level) {
  __shared__ int cur;
  if (threadIdx.x == 0) {
    const int i = min(*step + 1, n_steps - 1);
    *step = i;
    cur = i;
  }
  __syncthreads();
  const float nl = table[(size_t)DS_SOLVER_ROW * cur + 4];
  for (int b = threadIdx.x; b < B; b += 256) noise_level[b] = nl;
}

// post_process (sampling.py:53-97) with the inverse scaler of utils.py:88-103 (norms 1,4,4,1; centered).
__global__ void k_post_process(ds_layout L, const float* __restrict__ xh, const float* __restrict__ edge_x,
                               float* __restrict__ pos_out, int32_t* __restrict__ atom_type, int32_t* __restrict__ fc,
                               float* __restrict__ edge_type) {
  const int m = blockIdx.x, tid = threadIdx.x;
  const int n0 = L.node_off[m], n = L.node_off[m + 1] - n0;
  const int N = L.N;
  for (int a = tid; a < n; a += blockDim.x) {
    const size_t d = (size_t)L.node_dense[n0 + a];
    const float* r = xh + d * 9;
    pos_out[d * 3 + 0] = r[0] * 1.0f; pos_out[d * 3 + 1] = r[1] * 1.0f; pos_out[d * 3 + 2] = r[2] * 1.0f;
    int best = 0;
    float bv = (r[3] * 4.0f + 1.0f) / 2.0f;
    for (int t = 1; t < 5; ++t) {
      const float v = (r[3 + t] * 4.0f + 1.0f) / 2.0f;
      if (v > bv) { bv = v; best = t; }
    }
    atom_type[d] = best;
    fc[d] = (int32_t)rintf(r[8] * 4.0f);
  }
  for (int idx = tid; idx < n * n; idx += blockDim.x) {
    const int a = idx / n, b = idx - a * n;
    if (a == b) continue;
    const int da = L.node_dense[n0 + a], lb = L.node_dense[n0 + b] - m * N;
    const size_t o = (size_t)da * N + lb;
    const float ex = (edge_x[o * 2 + 0] * 1.0f + 1.0f) / 2.0f;
    const float t = ((edge_x[o * 2 + 1] * 1.0f + 1.0f) / 2.0f) * 3.0f;
    float et = 0.0f;
    if (t >= 2.5f) et = 3.0f; else if (t >= 1.5f) et = 2.0f; else if (t >= 0.5f) et = 1.0f;
    edge_type[o] = (ex >= 0.5f ? 1.0f : 0.0f) * et;
  }
}

// Stability check, one workgroup per molecule (evaluation/stability.py:40-73; tables of evaluation/bond_analyze.py:5-45 for
// H, C, N, O, F in ds_bonds.h, which the valence analytics on result records share).  Thread a walks the other atoms of its molecule.
using ds_bonds::c_valence;
__global__ __launch_bounds__(64) void k_check_stability(ds_layout L, const float* __restrict__ pos, const int32_t* __restrict__ atom_type,
                                                        int32_t* __restrict__ bond_order, int32_t* __restrict__ nr_stable,
                                                        int32_t* __restrict__ mol_stable) {
  __shared__ float px[32], py[32], pz[32];
  __shared__ int ty[32], dn[32];
  const int m = blockIdx.x, a = threadIdx.x;
  const int n0 = L.node_off[m], n = L.node_off[m + 1] - n0;
  if (n <= 0) { if (a == 0) { nr_stable[m] = 0; mol_stable[m] = 1; } return; }
  if (a < n) {
    const int d = L.node_dense[n0 + a];
    dn[a] = d;
    px[a] = pos[(size_t)d * 3]; py[a] = pos[(size_t)d * 3 + 1]; pz[a] = pos[(size_t)d * 3 + 2];
    ty[a] = min(max(atom_type[d], 0), 4);
  }
  __syncthreads();
  int ok = 0;
  if (a < n) {
    int bonds = 0;
    const int ta = ty[a], N = L.N;
    for (int b = 0; b < n; ++b) {
      if (b == a) continue;
      const float dx = px[a] - px[b], dy = py[a] - py[b], dz = pz[a] - pz[b];
      const float d = ds_bonds::scaled_distance(dx, dy, dz);
      const int order = ds_bonds::order_of(ta, ty[b], d);
      bonds += order;
      if (bond_order) bond_order[(size_t)dn[a] * N + (dn[b] - m * N)] = order;
    }
    ok = bonds == c_valence[ta] ? 1 : 0;
  }
  const int cnt = __popcll(__ballot(ok != 0));
  if (a == 0) { nr_stable[m] = cnt; mol_stable[m] = cnt == n ? 1 : 0; }
}

}  // namespace

extern "C" {

int ds_sampler_step(const ds_layout* L, float c_x, float c_pred, float sigma, float temperature, float* x, float* edge_x,
                     const float* pred, const float* edge_pred, const float* raw_pos, const float* raw_feat,
                     const float* raw_edge, float* x_mean, float* edge_mean, void* stream) {
  if (!layout_ok(L) || !x || !edge_x || !pred || !edge_pred || !raw_pos || !raw_feat || !raw_edge || !x_mean || !edge_mean) return DS_ERR_ARG;
  hipLaunchKernelGGL(k_sampler_step, dim3(L->B), dim3(256), 0, (hipStream_t)stream, *L, c_x, c_pred, sigma, temperature, x,
                     edge_x, pred, edge_pred, raw_pos, raw_feat, raw_edge, x_mean, edge_mean);
  return DST_CHECK_LAUNCH();
}

int ds_initial_noise(const ds_layout* L, uint64_t seed, const int64_t* mol_id, float* x, float* edge_x, void* stream) {
  if (!layout_ok(L) || !mol_id || !x || !edge_x) return DS_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const size_t nb = (size_t)L->B * L->N;
  if (!clear(x, nb * 9 * sizeof(float), s) || !clear(edge_x, nb * L->N * 2 * sizeof(float), s)) return DS_ERR_LAUNCH;
  hipLaunchKernelGGL(k_noise_step<0>, dim3(L->B), dim3(256), 0, s, *L, 0.0f, 0.0f, 0.0f, 0.0f, (unsigned long long)seed, 0u, mol_id,
                     x, edge_x, (const float*)nullptr, (const float*)nullptr, (float*)nullptr, (float*)nullptr,
                     (const float*)nullptr, (const int32_t*)nullptr);
  return DST_CHECK_LAUNCH();
}

int ds_sampler_step_philox(const ds_layout* L, float c_x, float c_pred, float sigma, float temperature, uint64_t seed, int32_t step,
                           const int64_t* mol_id, float* x, float* edge_x, const float* pred, const float* edge_pred,
                           float* x_mean, float* edge_mean, void* stream) {
  if (!layout_ok(L) || !mol_id || !x || !edge_x || !pred || !edge_pred || !x_mean || !edge_mean || step < 0) return DS_ERR_ARG;
  hipLaunchKernelGGL(k_noise_step<1>, dim3(L->B), dim3(256), 0, (hipStream_t)stream, *L, c_x, c_pred, sigma, temperature,
                     (unsigned long long)seed, (unsigned int)step + 1u, mol_id, x, edge_x, pred, edge_pred, x_mean, edge_mean,
                     (const float*)nullptr, (const int32_t*)nullptr);
  return DST_CHECK_LAUNCH();
}

int ds_step_begin(const float* table, int32_t n_steps, int32_t* step, int32_t B, float* noise_level, void* stream) {
  if (!table || !step || !noise_level || B <= 0 || n_steps <= 0) return DS_ERR_ARG;
  hipLaunchKernelGGL(k_step_begin, dim3(1), dim3(256), 0, (hipStream_t)stream, table, n_steps, step, B, noise_level);
  return DST_CHECK_LAUNCH();
}

int ds_sampler_step_philox_dev(const ds_layout* L, const float* table, const int32_t* step, float temperature, uint64_t seed,
                               const int64_t* mol_id, float* x, float* edge_x, const float* pred, const float* edge_pred,
                               float* x_mean, float* edge_mean, void* stream) {
  if (!layout_ok(L) || !table || !step || !mol_id || !x || !edge_x || !pred || !edge_pred || !x_mean || !edge_mean) return DS_ERR_ARG;
  hipLaunchKernelGGL(k_noise_step<2>, dim3(L->B), dim3(256), 0, (hipStream_t)stream, *L, 0.0f, 0.0f, 0.0f, temperature,
                     (unsigned long long)seed, 0u, mol_id, x, edge_x, pred, edge_pred, x_mean, edge_mean, table, step);
  return DST_CHECK_LAUNCH();
}

// ---- multistep solver update (include/diffspectra_solver.h) ----
int ds_solver_step(const ds_layout* L, float a, float b, float c, float d, float temperature, float* x, float* edge_x, const float* pred,
                   const float* edge_pred, const float* hist, const float* edge_hist, const float* raw_pos, const float* raw_feat,
                   const float* raw_edge, float* x_mean, float* edge_mean, void* stream) {
  if (!layout_ok(L) || !x || !edge_x || !pred || !edge_pred || !x_mean || !edge_mean) return DS_ERR_ARG;
  if (c != 0.0f && (!hist || !edge_hist)) return DS_ERR_ARG;
  if (d != 0.0f && (!raw_pos || !raw_feat || !raw_edge)) return DS_ERR_ARG;
  if (!edge_aligned8({edge_x, edge_pred, edge_hist, edge_mean})) return DS_ERR_ARG;
  hipLaunchKernelGGL(k_solver_step<0>, dim3(L->B), dim3(256), 0, (hipStream_t)stream, *L, a, b, c, d, temperature, 0ull, 0u,
                     (const int64_t*)nullptr, x, edge_x, pred, edge_pred, const_cast<float*>(hist), const_cast<float*>(edge_hist), raw_pos,
                     raw_feat, raw_edge, x_mean, edge_mean, (const float*)nullptr, (const int32_t*)nullptr);
  return DST_CHECK_LAUNCH();
}

int ds_solver_step_philox(const ds_layout* L, float a, float b, float c, float d, float temperature, uint64_t seed, int32_t step,
                          const int64_t* mol_id, float* x, float* edge_x, const float* pred, const float* edge_pred, const float* hist,
                          const float* edge_hist, float* x_mean, float* edge_mean, void* stream) {
  if (!layout_ok(L) || !mol_id || !x || !edge_x || !pred || !edge_pred || !x_mean || !edge_mean || step < 0) return DS_ERR_ARG;
  if (c != 0.0f && (!hist || !edge_hist)) return DS_ERR_ARG;
  if (!edge_aligned8({edge_x, edge_pred, edge_hist, edge_mean})) return DS_ERR_ARG;
  hipLaunchKernelGGL(k_solver_step<1>, dim3(L->B), dim3(256), 0, (hipStream_t)stream, *L, a, b, c, d, temperature,
                     (unsigned long long)seed, (unsigned int)step + 1u, mol_id, x, edge_x, pred, edge_pred, const_cast<float*>(hist),
                     const_cast<float*>(edge_hist), (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, x_mean, edge_mean,
                     (const float*)nullptr, (const int32_t*)nullptr);
  return DST_CHECK_LAUNCH();
}

int ds_solver_step_begin(const float* table, int32_t n_steps, int32_t* step, int32_t B, float* noise_level, void* stream) {
  if (!table || !step || !noise_level || B <= 0 || n_steps <= 0) return DS_ERR_ARG;
  hipLaunchKernelGGL(k_solver_step_begin, dim3(1), dim3(256), 0, (hipStream_t)stream, table, n_steps, step, B, noise_level);
  return DST_CHECK_LAUNCH();
}

int ds_solver_step_philox_dev(const ds_layout* L, const float* table, const int32_t* step, float temperature, uint64_t seed,
                              const int64_t* mol_id, float* x, float* edge_x, const float* pred, const float* edge_pred, float* hist,
                              float* edge_hist, float* x_mean, float* edge_mean, void* stream) {
  if (!layout_ok(L) || !table || !step || !mol_id || !x || !edge_x || !pred || !edge_pred || !hist || !edge_hist || !x_mean || !edge_mean)
    return DS_ERR_ARG;
  if (!edge_aligned8({edge_x, edge_pred, edge_hist, edge_mean})) return DS_ERR_ARG;
  hipLaunchKernelGGL(k_solver_step<2>, dim3(L->B), dim3(256), 0, (hipStream_t)stream, *L, 0.0f, 0.0f, 0.0f, 0.0f, temperature,
                     (unsigned long long)seed, 0u, mol_id, x, edge_x, pred, edge_pred, hist, edge_hist, (const float*)nullptr,
                     (const float*)nullptr, (const float*)nullptr, x_mean, edge_mean, table, step);
  return DST_CHECK_LAUNCH();
}

int ds_post_process(const ds_layout* L, const float* xh, const float* edge_x, float* pos_out, int32_t* atom_type, int32_t* fc,
                    float* edge_type, void* stream) {
  if (!layout_ok(L) || !xh || !edge_x || !pos_out || !atom_type || !fc || !edge_type) return DS_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const size_t nb = (size_t)L->B * L->N;
  if (!clear(pos_out, nb * 3 * sizeof(float), s) || !clear(atom_type, nb * sizeof(int32_t), s) || !clear(fc, nb * sizeof(int32_t), s) ||
      !clear(edge_type, nb * L->N * sizeof(float), s))
    return DS_ERR_LAUNCH;
  hipLaunchKernelGGL(k_post_process, dim3(L->B), dim3(128), 0, s, *L, xh, edge_x, pos_out, atom_type, fc, edge_type);
  return DST_CHECK_LAUNCH();
}

int ds_check_stability(const ds_layout* L, const float* pos, const int32_t* atom_type, int32_t* bond_order, int32_t* nr_stable,
                       int32_t* mol_stable, void* stream) {
  if (!layout_ok(L) || !pos || !atom_type || !nr_stable || !mol_stable) return DS_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (bond_order && !clear(bond_order, (size_t)L->B * L->N * L->N * sizeof(int32_t), s)) return DS_ERR_LAUNCH;
  hipLaunchKernelGGL(k_check_stability, dim3(L->B), dim3(64), 0, s, *L, pos, atom_type, bond_order, nr_stable, mol_stable);
  return DST_CHECK_LAUNCH();
}

}  // extern "C"
