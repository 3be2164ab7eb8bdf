// diffspectra_amd - maximum mean discrepancy of 1-D sample sets under a sum of Gaussian kernels, many (source, target) classes per call: the
// reference's compute_mmd (evaluation/mmd.py) behind its bond / angle / dihedral MMD.  ds_mmd_1d_segments in include/diffspectra_hip.h states
// the definition; DESIGN.md section 13 has the method and the figures.
//
// Three kernels on one stream, no floating-point atomics:
//   k_mmd_moments  one workgroup per class: validates the class's offsets, takes the mean and the centred second moment of the concatenation
//                  in fp64 (fixed thread stride, fixed tree) and leaves the bandwidth in the workspace;
//   k_mmd_pairs    grid (chunk, term XX | YY | XY, class), 256 threads: workgroup g takes the tiles g, g + CHUNKS, ... of its class and term.
//                  A tile is 256 rows x 256 columns: a row value per thread in a register, the column chunk in LDS and read as float4
//                  broadcasts (every lane reads the same address).  The work is VALU: per pair a subtract, two multiplies, one v_exp_f32 and,
//                  with kernel_mul = 2 and at most 5 bandwidths, one multiply and one add per bandwidth (exp(-d^2 / bw_k) is the square of
//                  exp(-d^2 / bw_(k+1)));
//                  otherwise a multiply, a v_exp_f32 and an add per bandwidth.  Each lane sums per bandwidth in fp32 over 64 columns, then
//                  in fp64; XX and YY skip the tiles below the diagonal and double those above it;
//   k_mmd_finish   one thread per class adds the CHUNKS partials of each term in index order and forms XX, YY, XY and mmd.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "../../include/diffspectra_hip.h"
#include "ds_host.h"   // DST_CHECK_LAUNCH

namespace {

constexpr int TILE = DS_MMD_TILE, CHUNKS = DS_MMD_CHUNKS, KMAX = DS_MMD_MAX_KERNELS;
constexpr int DOUBLING_MAX = 5;                            // bandwidths one exponential may serve: four squarings, each doubles the relative error
constexpr int RUN = 64;                                    // columns a lane sums in fp32 before it goes to fp64
constexpr int WS_PER_CLASS = 2 + 3 * CHUNKS;               // doubles: bandwidth, pad, partial[term][chunk]
static_assert(TILE == 256 && TILE % RUN == 0 && RUN % 4 == 0, "a row per thread of a 256-thread workgroup, float4 column reads");

struct Segment {
  int64_t lo, n;                                           // first sample and number of samples; n < 0: the offsets are not usable
};

__device__ __forceinline__ Segment segment_of(const int64_t* __restrict__ off, int64_t c, int64_t total) {
  const int64_t lo = off[c], hi = off[c + 1];
  if (lo < 0 || hi < lo || hi > total || hi - lo > DS_MMD_MAX_SAMPLES) return {0, -1};
  return {lo, hi - lo};
}

// sum of v over the workgroup in a fixed order, in every thread
__device__ double block_sum(double v, double* __restrict__ sh, int tid) {
  __syncthreads();
  sh[tid] = v;
  __syncthreads();
  for (int s = TILE / 2; s; s >>= 1) {
    if (tid < s) sh[tid] += sh[tid + s];
    __syncthreads();
  }
  return sh[0];
}

__global__ __launch_bounds__(TILE) void k_mmd_moments(const float* __restrict__ x, const int64_t* __restrict__ x_off, int64_t Nx,
                                                      const float* __restrict__ y, const int64_t* __restrict__ y_off, int64_t Ny,
                                                      double fix_sigma, double* __restrict__ ws, unsigned char* __restrict__ status) {
  __shared__ double sh[TILE];
  const int64_t c = blockIdx.x;
  const int tid = threadIdx.x;
  const Segment a = segment_of(x_off, c, Nx), b = segment_of(y_off, c, Ny);
  double* __restrict__ mine = ws + c * WS_PER_CLASS;
  if (a.n <= 0 || b.n <= 0) {                              // the same in every thread
    if (tid == 0) {
      mine[0] = __builtin_nan("");
      status[c] = (a.n < 0 || b.n < 0) ? DS_MMD_INVALID : DS_MMD_EMPTY;
    }
    return;
  }
  double bw = fix_sigma;
  if (!(fix_sigma > 0.0)) {
    const double N = (double)(a.n + b.n);
    double s = 0.0;
    for (int64_t i = tid; i < a.n; i += TILE) s += (double)x[a.lo + i];
    for (int64_t i = tid; i < b.n; i += TILE) s += (double)y[b.lo + i];
    const double mean = block_sum(s, sh, tid) / N;
    double m2 = 0.0;
    for (int64_t i = tid; i < a.n; i += TILE) { const double d = (double)x[a.lo + i] - mean; m2 += d * d; }
    for (int64_t i = tid; i < b.n; i += TILE) { const double d = (double)y[b.lo + i] - mean; m2 += d * d; }
    bw = 2.0 * block_sum(m2, sh, tid) / (N - 1.0);         // sum_ij (z_i - z_j)^2 / (N^2 - N)
  }
  if (tid == 0) { mine[0] = bw; status[c] = DS_MMD_OK; }
}

template <int KN, bool DOUBLING>
__global__ __launch_bounds__(TILE) void k_mmd_pairs(const float* __restrict__ x, const int64_t* __restrict__ x_off, int64_t Nx,
                                                    const float* __restrict__ y, const int64_t* __restrict__ y_off, int64_t Ny,
                                                    double kernel_mul, double* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) float col[TILE];
  __shared__ double sh[TILE];
  const int g = blockIdx.x, term = blockIdx.y;             // term 0: XX, 1: YY, 2: XY
  const int64_t c = blockIdx.z;
  const int tid = threadIdx.x;
  const Segment a = segment_of(x_off, c, Nx), b = segment_of(y_off, c, Ny);
  if (a.n <= 0 || b.n <= 0) return;                        // k_mmd_finish does not read this class's partials
  double* __restrict__ mine = ws + c * WS_PER_CLASS;
  // -log2(e) / bw_k, bw_k = bandwidth / mul^(KN / 2) * mul^k
  float scale[KN];
  {
    double bw = mine[0];
    for (int k = 0; k < KN / 2; ++k) bw /= kernel_mul;
#pragma unroll
    for (int k = 0; k < KN; ++k) { scale[k] = (float)(-1.4426950408889634074 / bw); bw *= kernel_mul; }
  }
  const Segment rows = term == 1 ? b : a, cols = term == 0 ? a : b;
  const float* __restrict__ row_v = (term == 1 ? y : x) + rows.lo;
  const float* __restrict__ col_v = (term == 0 ? x : y) + cols.lo;
  const int64_t tr = (rows.n + TILE - 1) / TILE, tc = (cols.n + TILE - 1) / TILE;
  double total = 0.0;
  for (int64_t t = g; t < tr * tc; t += CHUNKS) {
    const int64_t rt = t / tc, ct = t - rt * tc;
    if (term != 2 && ct < rt) continue;                    // the lower triangle is the upper one again
    const int64_t c0 = ct * TILE, r = rt * TILE + tid;
    const int width = cols.n - c0 < TILE ? (int)(cols.n - c0) : TILE;
    __syncthreads();
    col[tid] = tid < width ? col_v[c0 + tid] : __builtin_inff();       // d = -inf, d^2 * scale = -inf, exp2 = 0: no term
    __syncthreads();
    const bool held = r < rows.n;
    const float xr = held ? row_v[r] : 0.0f;
    double sum = 0.0;
    for (int q = 0; q < width; q += RUN) {
      float acc[KN];
#pragma unroll
      for (int k = 0; k < KN; ++k) acc[k] = 0.0f;
#pragma unroll 4
      for (int j = q; j < q + RUN; j += 4) {
        const float4 v4 = *reinterpret_cast<const float4*>(col + j);
        const float v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float d = xr - v[u], s = d * d;
          if (DOUBLING) {
            float e = __builtin_amdgcn_exp2f(s * scale[KN - 1]);
            acc[KN - 1] += e;
#pragma unroll
            for (int k = KN - 2; k >= 0; --k) { e *= e; acc[k] += e; }
          } else {
#pragma unroll
            for (int k = 0; k < KN; ++k) acc[k] += __builtin_amdgcn_exp2f(s * scale[k]);
          }
        }
      }
#pragma unroll
      for (int k = 0; k < KN; ++k) sum += (double)acc[k];
    }
    if (held) total += (term != 2 && ct != rt) ? 2.0 * sum : sum;
  }
  total = block_sum(total, sh, tid);
  if (tid == 0) mine[2 + term * CHUNKS + g] = total;
}

__global__ __launch_bounds__(64) void k_mmd_finish(const int64_t* __restrict__ x_off, const int64_t* __restrict__ y_off, int64_t C,
                                                   const double* __restrict__ ws, const unsigned char* __restrict__ status,
                                                   double* __restrict__ out) {
  const int64_t c = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (c >= C) return;
  const double* __restrict__ mine = ws + c * WS_PER_CLASS;
  const double nan = __builtin_nan("");
  double* __restrict__ o = out + c * 5;
  const double bw = mine[0];
  if (status[c] != DS_MMD_OK || !(bw > 0.0) || !isfinite(bw)) {
    o[0] = nan; o[1] = nan; o[2] = nan; o[3] = nan; o[4] = status[c] == DS_MMD_OK ? bw : nan;
    return;
  }
  const double ns = (double)(x_off[c + 1] - x_off[c]), nt = (double)(y_off[c + 1] - y_off[c]);
  double s[3];
  for (int term = 0; term < 3; ++term) {
    double v = 0.0;
    for (int g = 0; g < CHUNKS; ++g) v += mine[2 + term * CHUNKS + g];
    s[term] = v;
  }
  const double xx = s[0] / (ns * ns), yy = s[1] / (nt * nt), xy = s[2] / (ns * nt);
  o[0] = xx + yy - 2.0 * xy; o[1] = xx; o[2] = yy; o[3] = xy; o[4] = bw;
}

template <int KN>
void launch_pairs(bool doubling, dim3 grid, hipStream_t st, const float* x, const int64_t* x_off, int64_t Nx, const float* y,
                  const int64_t* y_off, int64_t Ny, double mul, double* ws) {
  if constexpr (KN <= DOUBLING_MAX) {
    if (doubling) {
      hipLaunchKernelGGL((k_mmd_pairs<KN, true>), grid, dim3(TILE), 0, st, x, x_off, Nx, y, y_off, Ny, mul, ws);
      return;
    }
  }
  hipLaunchKernelGGL((k_mmd_pairs<KN, false>), grid, dim3(TILE), 0, st, x, x_off, Nx, y, y_off, Ny, mul, ws);
}

}  // namespace

extern "C" int ds_mmd_1d_workspace_bytes(int64_t n_classes, int64_t* bytes) {
  if (n_classes < 0 || n_classes > DS_MMD_MAX_CLASSES || !bytes) return DS_ERR_ARG;
  *bytes = n_classes * WS_PER_CLASS * (int64_t)sizeof(double);
  return DS_OK;
}

extern "C" int ds_mmd_1d_segments(const float* x, const int64_t* x_off, int64_t Nx, const float* y, const int64_t* y_off, int64_t Ny,
                                  int64_t n_classes, double kernel_mul, int32_t kernel_num, double fix_sigma, void* workspace,
                                  int64_t workspace_bytes, double* out, uint8_t* status, void* stream) {
  const int64_t C = n_classes;
  if (C < 0 || C > DS_MMD_MAX_CLASSES || Nx < 0 || Nx > 0x7fffffffll || Ny < 0 || Ny > 0x7fffffffll) return DS_ERR_ARG;
  if (kernel_num < 1 || kernel_num > KMAX || !std::isfinite(kernel_mul) || !(kernel_mul > 0.0)) return DS_ERR_ARG;
  if (!std::isfinite(fix_sigma) || fix_sigma < 0.0) return DS_ERR_ARG;
  if (C == 0) return DS_OK;
  if (!x_off || !y_off || !out || !status || !workspace || (Nx > 0 && !x) || (Ny > 0 && !y)) return DS_ERR_ARG;
  if (workspace_bytes < C * WS_PER_CLASS * (int64_t)sizeof(double) || reinterpret_cast<uintptr_t>(workspace) & 7) return DS_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  double* ws = static_cast<double*>(workspace);
  hipLaunchKernelGGL(k_mmd_moments, dim3((unsigned)C), dim3(TILE), 0, st, x, x_off, Nx, y, y_off, Ny, fix_sigma, ws, status);
  const dim3 grid(CHUNKS, 3, (unsigned)C);
  const bool doubling = kernel_mul == 2.0;                  // launch_pairs uses it up to DOUBLING_MAX bandwidths
  switch (kernel_num) {
    case 1: launch_pairs<1>(false, grid, st, x, x_off, Nx, y, y_off, Ny, kernel_mul, ws); break;
    case 2: launch_pairs<2>(doubling, grid, st, x, x_off, Nx, y, y_off, Ny, kernel_mul, ws); break;
    case 3: launch_pairs<3>(doubling, grid, st, x, x_off, Nx, y, y_off, Ny, kernel_mul, ws); break;
    case 4: launch_pairs<4>(doubling, grid, st, x, x_off, Nx, y, y_off, Ny, kernel_mul, ws); break;
    case 5: launch_pairs<5>(doubling, grid, st, x, x_off, Nx, y, y_off, Ny, kernel_mul, ws); break;
    case 6: launch_pairs<6>(doubling, grid, st, x, x_off, Nx, y, y_off, Ny, kernel_mul, ws); break;
    case 7: launch_pairs<7>(doubling, grid, st, x, x_off, Nx, y, y_off, Ny, kernel_mul, ws); break;
    default: launch_pairs<8>(doubling, grid, st, x, x_off, Nx, y, y_off, Ny, kernel_mul, ws); break;
  }
  hipLaunchKernelGGL(k_mmd_finish, dim3((unsigned)((C + 63) / 64)), dim3(64), 0, st, x_off, y_off, C, ws, status, out);
  return DST_CHECK_LAUNCH();
}
