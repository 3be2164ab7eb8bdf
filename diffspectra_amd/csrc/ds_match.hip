// diffspectra_amd - structure metric of the evaluation path: Hungarian-matched RMSD, atom-type / bond accuracy and the certified
// exact-graph flag of (generated, ground-truth) molecule pairs, one wave64 per pair, fp64 throughout (ds_match_records in
// include/diffspectra_hip.h states the semantics; they restate eval_sampled_mols/rmsd.py:12-73,106-128,153-227 of the reference).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/diffspectra_hip.h"
#include "ds_records.h"
#include "ds_svd3.h"
#include "ds_host.h"   // DST_CHECK_LAUNCH

namespace {

using ds_rec::MA;                         // 29 atoms: lanes 0..28 are atoms / assignment columns
using ds_rec::uniform_i;

__device__ __forceinline__ double uniform_d(double v) {
  const long long b = __double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)b), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(b >> 32));
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
// sum over the 32 low lanes (atoms live in lanes 0..28; the others contribute what they hold, so they pass 0), returned uniform
__device__ __forceinline__ int sum32_i(int v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return uniform_i(v);
}
__device__ __forceinline__ double sum32_d(double v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return uniform_d(v);
}

struct Side {                       // one molecule of the pair in LDS
  unsigned char bond[MA * MA + 7];  // bond orders of the record, original atom indices; bond(i, j) is read from the upper triangle
  unsigned char type[32], orig[32]; // per FRAGMENT atom: decoder type, original atom index
  signed char fc[32];
  double x[32][3];                  // per fragment atom: centred coordinates (generated side: rotated in place after the Kabsch fit)
  unsigned reach[32];               // per ORIGINAL atom: bit mask of the atoms it is connected to (scratch of the fragment search)
  int n, nf;                        // atoms of the molecule, atoms of its largest fragment
};

__device__ __forceinline__ int bond_of(const Side& s, int i, int j) { return s.bond[min(i, j) * MA + max(i, j)]; }

// Largest connected fragment (a bond is an order > 0; ties: the fragment that holds the lowest atom index; fragment atoms keep ascending
// original order), its coordinates centred on its own centroid.  Lane = original atom.
__device__ void load_side(Side& s, const unsigned char* __restrict__ rec, int n, int lane) {
  for (int k = lane; k < MA * MA; k += 64) s.bond[k] = rec[DS_REC_BOND + k];
  if (lane == 0) s.n = n;
  __syncthreads();
  unsigned mine = 0;
  if (lane < n) {
    mine = 1u << lane;
    for (int j = 0; j < n; ++j)
      if (j != lane && bond_of(s, lane, j) > 0) mine |= 1u << j;
  }
  if (lane < 32) s.reach[lane] = mine;
  __syncthreads();
  for (int round = 0; round < 5; ++round) {          // paths double in length every round: 2^5 >= 29
    unsigned next = mine;
    for (unsigned m = mine; m; m &= m - 1) next |= s.reach[__ffs(m) - 1];
    __syncthreads();
    mine = next;
    if (lane < 32) s.reach[lane] = mine;
    __syncthreads();
  }
  // largest fragment, lowest first atom on ties: maximise size * 32 + (31 - first atom)
  int key = lane < n ? __popc(mine) * 32 + (31 - (__ffs(mine) - 1)) : -1;
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) key = max(key, __shfl_xor(key, o, 64));
  key = uniform_i(key);
  const unsigned frag = n > 0 ? s.reach[31 - (key & 31)] : 0u;
  const int nf = __popc(frag);
  const bool in = lane < n && ((frag >> lane) & 1u);
  const int k = __popc(frag & ((1u << (lane & 31)) - 1u));           // fragment position of atom `lane`
  double p[3] = {0.0, 0.0, 0.0};
  if (in) {
    const float* pos = reinterpret_cast<const float*>(rec) + lane * 3;
    p[0] = (double)pos[0]; p[1] = (double)pos[1]; p[2] = (double)pos[2];
    s.type[k] = rec[DS_REC_TYPE + lane];
    s.fc[k] = (signed char)rec[DS_REC_FC + lane];
    s.orig[k] = (unsigned char)lane;
    s.x[k][0] = p[0]; s.x[k][1] = p[1]; s.x[k][2] = p[2];
  }
  if (lane == 0) s.nf = nf;
  __syncthreads();
  double c[3] = {0.0, 0.0, 0.0};                               // centroid: ascending fragment order, the same sum in every lane
  for (int a = 0; a < nf; ++a) { c[0] += s.x[a][0]; c[1] += s.x[a][1]; c[2] += s.x[a][2]; }
  __syncthreads();
  if (in) {
    const double inv = (double)nf;
    s.x[k][0] = p[0] - c[0] / inv; s.x[k][1] = p[1] - c[1] / inv; s.x[k][2] = p[2] - c[2] / inv;
  }
  __syncthreads();
}

// cost[p][r] = |x_p - x_r| + type penalty (0 same type, 2 both in {C, N, O}, 10 otherwise); entries above `clip` become 1000
__device__ void build_cost(double* __restrict__ cost, const Side& g, const Side& t, double clip, bool clipped, int lane) {
  const int np = g.nf, nr = t.nf;
  for (int e = lane; e < np * nr; e += 64) {
    const int i = e / nr, j = e - i * nr;
    const double dx = g.x[i][0] - t.x[j][0], dy = g.x[i][1] - t.x[j][1], dz = g.x[i][2] - t.x[j][2];
    const int a = g.type[i], b = t.type[j];
    const double pen = a == b ? 0.0 : ((a >= 1 && a <= 3 && b >= 1 && b <= 3) ? 2.0 : 10.0);
    double c = sqrt(dx * dx + dy * dy + dz * dz) + pen;
    if (clipped && c > clip) c = 1000.0;
    cost[i * MA + j] = c;
  }
  __syncthreads();
}

// Minimum-cost assignment of the np x nr cost matrix by shortest augmenting paths (the potentials form of the Hungarian method): rows =
// the smaller side, lane = column of the larger side, one wave-wide arg-min (lowest column on ties) per step of a path.  Every row of
// the smaller side ends up assigned.  match[p] = column r of generated fragment atom p, or -1.
__device__ void assign(const double* __restrict__ cost, int np, int nr, double* __restrict__ u, int* __restrict__ match, int lane) {
  const bool T = np > nr;                                    // transposed: rows are ground-truth atoms, lanes generated atoms
  const int nrows = T ? nr : np, ncols = T ? np : nr;
  const bool col = lane < ncols;
  const double INF = __longlong_as_double(0x7ff0000000000000ll);
  double v = 0.0;                                            // column potential
  int owner = -1;                                            // row assigned to this lane's column
  if (lane < 32) { u[lane] = 0.0; match[lane] = -1; }
  __syncthreads();
  for (int i = 0; i < nrows; ++i) {
    double minv = INF;
    int way = -1;
    bool used = false;
    int j0 = -1, i0 = i;                                     // j0 = -1: the virtual column that holds the new row
    for (int guard = 0; guard <= ncols; ++guard) {
      const double ui0 = u[i0];
      if (col && !used) {
        const double cur = (T ? cost[lane * MA + i0] : cost[i0 * MA + lane]) - ui0 - v;
        if (cur < minv) { minv = cur; way = j0; }
      }
      double best = (col && !used) ? minv : INF;
      int arg = lane;
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) {
        const double ob = __shfl_xor(best, o, 64);
        const int oa = __shfl_xor(arg, o, 64);
        if (ob < best || (ob == best && oa < arg)) { best = ob; arg = oa; }
      }
      const double delta = uniform_d(best);
      const int j1 = uniform_i(arg);
      if (!(delta < INF)) break;                             // (no free column: cannot happen with nrows <= ncols and finite costs)
      __syncthreads();                                       // every lane has read u[i0]
      if (col && used) { u[owner] += delta; v -= delta; }
      else if (col) minv -= delta;
      if (lane == 0) u[i] += delta;
      __syncthreads();
      j0 = j1;
      if (lane == j0) used = true;
      i0 = uniform_i(__shfl(owner, j0, 64));
      if (i0 < 0) break;                                     // a free column: the path ends
    }
    for (int guard = 0; guard <= ncols && j0 >= 0; ++guard) {   // flip the path back to the virtual column
      const int j1 = uniform_i(__shfl(way, j0, 64));
      const int pj1 = uniform_i(__shfl(owner, max(j1, 0), 64));
      if (lane == j0) owner = j1 >= 0 ? pj1 : i;
      j0 = j1;
    }
  }
  if (col && owner >= 0) {
    if (T) match[lane] = owner; else match[owner] = lane;
  }
  __syncthreads();
}

__global__ __launch_bounds__(64) void k_match_records(const unsigned char* __restrict__ prb_rec, const int32_t* __restrict__ prb_n,
                                                      const unsigned char* __restrict__ ref_rec, const int32_t* __restrict__ ref_n,
                                                      const int64_t* __restrict__ ref_index, int64_t M, float max_distance, int min_atoms,
                                                      double* __restrict__ rmsd, int32_t* __restrict__ n_matched, float* __restrict__ type_acc,
                                                      float* __restrict__ bond_acc, unsigned char* __restrict__ exact, int32_t* __restrict__ map) {
  __shared__ Side G, R_;                                     // generated ("probe") and ground-truth ("reference") molecule
  __shared__ double cost[MA * MA];
  __shared__ double u[32];
  __shared__ int match[32];
  const int64_t p = blockIdx.x;
  const int lane = threadIdx.x;
  const ds_rec::Pair q = ds_rec::pair_of(p, prb_rec, prb_n, ref_rec, ref_n, ref_index, M);
  const double NaN = __longlong_as_double(0x7ff8000000000000ll);
  int count = 0;
  bool valid = q.valid;
  if (valid) {
    load_side(G, q.prb, q.n_prb(), lane);
    load_side(R_, q.ref, q.n_ref(), lane);
    valid = min(G.nf, R_.nf) >= max(min_atoms, 1);           // the unclipped first match assigns every atom of the smaller fragment
    // a fragment with a non-finite coordinate (a diverged sample) has no cost matrix: the pair is invalid, as the reference's assignment
    // refuses such a matrix (rmsd.py:164-168).  Centring spreads one bad value over the whole fragment, so every lane sees it.
    bool finite = true;
    if (lane < G.nf) finite = isfinite(G.x[lane][0]) && isfinite(G.x[lane][1]) && isfinite(G.x[lane][2]);
    if (lane < R_.nf) finite = finite && isfinite(R_.x[lane][0]) && isfinite(R_.x[lane][1]) && isfinite(R_.x[lane][2]);
    valid = valid && __ballot(!finite) == 0ull;
  }
  double out_rmsd = NaN;
  float out_type = 0.0f, out_bond = 0.0f;
  int out_exact = 0, out_map = -1;
  if (valid) {
    const int np = G.nf, nr = R_.nf;
    build_cost(cost, G, R_, 0.0, false, lane);
    assign(cost, np, nr, u, match, lane);
    // Kabsch on the matched rows, ascending generated index: H = P^T Q = U S V^T, rot = U V^T (last singular direction negated if det < 0)
    double H[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, U[3][3], S[3], V[3][3], rot[3][3];
    for (int k = 0; k < np; ++k) {
      const int m = match[k];
      if (m < 0) continue;
      for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) H[a][b] += G.x[k][a] * R_.x[m][b];
    }
    svd3(H, U, S, V);
    double sg = 1.0;
    for (int pass = 0; pass < 2; ++pass) {
      for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) rot[a][b] = U[a][0] * V[b][0] + U[a][1] * V[b][1] + sg * U[a][2] * V[b][2];
      const double det = rot[0][0] * (rot[1][1] * rot[2][2] - rot[1][2] * rot[2][1]) - rot[0][1] * (rot[1][0] * rot[2][2] - rot[1][2] * rot[2][0]) +
                         rot[0][2] * (rot[1][0] * rot[2][1] - rot[1][1] * rot[2][0]);
      if (pass == 1 || !(det < 0.0)) break;
      sg = -1.0;
    }
    __syncthreads();
    if (lane < np) {                                         // aligned = centred_generated . rot
      const double x = G.x[lane][0], y = G.x[lane][1], z = G.x[lane][2];
      for (int b = 0; b < 3; ++b) G.x[lane][b] = x * rot[0][b] + y * rot[1][b] + z * rot[2][b];
    }
    __syncthreads();
    const bool clipped = isfinite(max_distance);
    const double clip = (double)max_distance;
    build_cost(cost, G, R_, clip, clipped, lane);
    assign(cost, np, nr, u, match, lane);
    // keep the matches whose (clipped) cost is within max_distance; lane = generated fragment atom
    int m = lane < np ? match[lane] : -1;
    if (m >= 0 && clipped && !(cost[lane * MA + m] <= clip)) m = -1;
    __syncthreads();
    if (lane < 32) match[lane] = m;
    __syncthreads();
    count = sum32_i(m >= 0 ? 1 : 0);
    valid = count >= max(min_atoms, 1);
    if (valid) {
      double d2 = 0.0;
      int same_type = 0, same_fc = 0, pairs = 0, same_bond = 0;
      if (m >= 0) {
        const double dx = G.x[lane][0] - R_.x[m][0], dy = G.x[lane][1] - R_.x[m][1], dz = G.x[lane][2] - R_.x[m][2];
        d2 = dx * dx + dy * dy + dz * dz;
        same_type = G.type[lane] == R_.type[m];
        same_fc = G.fc[lane] == R_.fc[m];
        for (int b = lane + 1; b < np; ++b) {
          const int mb = match[b];
          if (mb < 0) continue;
          ++pairs;
          same_bond += bond_of(G, G.orig[lane], G.orig[b]) == bond_of(R_, R_.orig[m], R_.orig[mb]);
        }
      }
      const double ss = sum32_d(d2);
      const int n_type = sum32_i(same_type), n_fc = sum32_i(same_fc), n_pairs = sum32_i(pairs), n_bond = sum32_i(same_bond);
      out_rmsd = sqrt(ss / (double)count);
      out_type = (float)((double)n_type / (double)count);
      out_bond = n_pairs > 0 ? (float)((double)n_bond / (double)n_pairs) : 0.0f;
      out_exact = np == G.n && nr == R_.n && np == nr && count == np && n_type == count && n_fc == count && n_bond == n_pairs;
      // the map speaks original atom indices: generated atom `lane` -> ground-truth atom
      for (int k = 0; k < np; ++k)
        if (G.orig[k] == lane && match[k] >= 0) out_map = R_.orig[match[k]];
    }
  }
  if (lane < MA) map[p * MA + lane] = out_map;
  if (lane == 0) {
    rmsd[p] = out_rmsd;
    n_matched[p] = count;
    type_acc[p] = out_type;
    bond_acc[p] = out_bond;
    exact[p] = (unsigned char)out_exact;
  }
}

}  // namespace

extern "C" int ds_match_records(const uint8_t* prb_rec, const int32_t* prb_n, int64_t P, const uint8_t* ref_rec, const int32_t* ref_n, int64_t M,
                                const int64_t* ref_index, float max_distance, int32_t min_atoms, double* rmsd, int32_t* n_matched,
                                float* type_acc, float* bond_acc, uint8_t* exact, int32_t* map, void* stream) {
  const int go = ds_rec::check_pairs(max_distance == max_distance, P, M, prb_rec, prb_n, ref_rec, ref_n, ref_index,
                                     {rmsd, n_matched, type_acc, bond_acc, exact, map});
  if (go != ds_rec::LAUNCH) return go;
  hipLaunchKernelGGL(k_match_records, dim3((unsigned)P), dim3(64), 0, (hipStream_t)stream, prb_rec, prb_n, ref_rec, ref_n, ref_index, M,
                     max_distance, (int)min_atoms, rmsd, n_matched, type_acc, bond_acc, exact, map);
  return DST_CHECK_LAUNCH();
}
