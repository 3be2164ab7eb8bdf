// diffspectra_amd - bond lengths, bond angles and dihedral angles of result records, sorted into caller-listed substructure classes: the sample
// lists of the reference's bond / angle / dihedral MMD (ds_geometry_count_records and ds_geometry_fill_records in include/diffspectra_hip.h
// state the definition, the class encoding and the deviations from the reference; DESIGN.md section 13 has the method and the figures).
//
// One wave64 per record and per workgroup, an atom per lane (lanes 29..63 hold none), no atomics.  Lane i walks what the header's order gives
// it - the bonds i < j, the angles centred on i, the dihedrals whose lower middle atom is i - always in the same lexicographic order, so the
// count kernel, the counting pass of the fill kernel and its writing pass see the same entries; a wave prefix sum over the lanes' counts
// places every lane's run inside the record's.  A class is matched before the value is computed, and the value (fp64, no fused multiply-add:
// reading an entry backwards gives the same bits) decides whether the entry is emitted or counted in `skipped`.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/diffspectra_hip.h"
#include "ds_records.h"
#include "ds_host.h"   // DST_CHECK_LAUNCH

namespace {

using ds_rec::MA;
constexpr int NC = DS_GEOM_MAX_CLASSES;
constexpr double DEG = 57.295779513082320877;              // 180 / pi
static_assert(NC == 32, "a class table is loaded by the lanes 0..31");

struct Mol {                                               // one record in LDS; arrays of 32 are indexed by atom
  double pos[32][3];
  int tbl[3][NC];                                          // class codes of the three kinds, -1 beyond a table's end (no code is negative)
  unsigned nb[32];                                         // bonded neighbours of every atom
  unsigned char adj[MA * 32];
  unsigned char type[32];
};

// position of the first class whose code is the entry's fields read forwards or backwards, or -1
__device__ __forceinline__ int class_of(const int* __restrict__ tbl, unsigned fwd, unsigned rev) {
  for (int k = 0; k < NC; ++k) {
    const int t = tbl[k];                                  // a negative code (the padding, or a caller's) equals no entry's
    if (t == (int)fwd || t == (int)rev) return k;
  }
  return -1;
}

__device__ __forceinline__ bool bond_value(const double* a, const double* b, float& out) {
#pragma clang fp contract(off)
  const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
  const double s = (dx * dx + dy * dy) + dz * dz;
  const double d = sqrt(s);
  out = (float)d;
  return s > 0.0 && isfinite(d);
}

__device__ __forceinline__ bool angle_value(const double* a, const double* c, const double* b, float& out) {
#pragma clang fp contract(off)
  const double ux = a[0] - c[0], uy = a[1] - c[1], uz = a[2] - c[2];
  const double vx = b[0] - c[0], vy = b[1] - c[1], vz = b[2] - c[2];
  const double uu = (ux * ux + uy * uy) + uz * uz, vv = (vx * vx + vy * vy) + vz * vz, uv = (ux * vx + uy * vy) + uz * vz;
  const double den = sqrt(uu * vv);
  if (!(den > 0.0) || !isfinite(den)) { out = 0.0f; return false; }
  const double cs = fmin(fmax(uv / den, -1.0), 1.0);
  const double deg = acos(cs) * DEG;
  out = (float)deg;
  return isfinite(deg);                                    // a NaN cosine (non-finite coordinates) ends here
}

__device__ __forceinline__ bool dihedral_value(const double* a, const double* i, const double* j, const double* b, float& out) {
#pragma clang fp contract(off)
  const double b1x = i[0] - a[0], b1y = i[1] - a[1], b1z = i[2] - a[2];
  const double b2x = j[0] - i[0], b2y = j[1] - i[1], b2z = j[2] - i[2];
  const double b3x = b[0] - j[0], b3y = b[1] - j[1], b3z = b[2] - j[2];
  const double n1x = b1y * b2z - b1z * b2y, n1y = b1z * b2x - b1x * b2z, n1z = b1x * b2y - b1y * b2x;
  const double n2x = b2y * b3z - b2z * b3y, n2y = b2z * b3x - b2x * b3z, n2z = b2x * b3y - b2y * b3x;
  const double n1n1 = (n1x * n1x + n1y * n1y) + n1z * n1z, n2n2 = (n2x * n2x + n2y * n2y) + n2z * n2z;
  const double b2b2 = (b2x * b2x + b2y * b2y) + b2z * b2z;
  out = 0.0f;
  if (!(n1n1 > 0.0) || !(n2n2 > 0.0) || !(b2b2 > 0.0)) return false;
  const double mx = n1y * n2z - n1z * n2y, my = n1z * n2x - n1x * n2z, mz = n1x * n2y - n1y * n2x;
  const double x = (n1x * n2x + n1y * n2y) + n1z * n2z;
  const double y = ((mx * b2x + my * b2y) + mz * b2z) / sqrt(b2b2);
  const double deg = atan2(y, x) * DEG;
  const float f = (float)deg;
  out = f <= -180.0f ? 180.0f : f;
  return isfinite(deg);
}

// What a pass does with an emitted entry: the counting passes only count, the writing pass stores at the lane's running position.
struct Sink {
  float* value[3];
  unsigned char* cls[3];
  int64_t at[3], total[3];                                 // next index of this lane per kind; the length of each kind's output
};

// The entries of lane `me` (an atom below n), in the header's order.  cnt[kind] counts the emitted ones, `skipped` the listed-but-undefined.
template <bool WRITE>
__device__ void walk(const Mol& M, int me, int (&cnt)[3], int& skipped, Sink& out) {
  auto emit = [&](int kind, int k, bool ok, float v) {
    if (!ok) { ++skipped; return; }
    if (WRITE) {
      const int64_t at = out.at[kind]++;
      if (at >= 0 && at < out.total[kind]) { out.value[kind][at] = v; out.cls[kind][at] = (unsigned char)k; }
    }
    ++cnt[kind];
  };
  const unsigned nb = M.nb[me];
  const unsigned ti = M.type[me];
  const unsigned char* __restrict__ row = M.adj + me * 32;
  // bonds me < j
  for (unsigned r = nb & ~((2u << me) - 1u); r; r &= r - 1u) {
    const int j = __ffs(r) - 1;
    const unsigned tj = M.type[j], o = row[j];
    if ((ti | tj | o) > 15u) continue;
    const int k = class_of(M.tbl[0], ti | o << 4 | tj << 8, tj | o << 4 | ti << 8);
    if (k < 0) continue;
    float v;
    const bool ok = bond_value(M.pos[me], M.pos[j], v);
    emit(0, k, ok, v);
  }
  // angles a - me - b, a < b
  for (unsigned ra = nb; ra; ra &= ra - 1u) {
    const int a = __ffs(ra) - 1;
    const unsigned ta = M.type[a], oa = row[a];
    for (unsigned rb = ra & (ra - 1u); rb; rb &= rb - 1u) {
      const int b = __ffs(rb) - 1;
      const unsigned tb = M.type[b], ob = row[b];
      if ((ta | oa | ti | ob | tb) > 15u) continue;
      const int k = class_of(M.tbl[1], ta | oa << 4 | ti << 8 | ob << 12 | tb << 16, tb | ob << 4 | ti << 8 | oa << 12 | ta << 16);
      if (k < 0) continue;
      float v;
      const bool ok = angle_value(M.pos[a], M.pos[me], M.pos[b], v);
      emit(1, k, ok, v);
    }
  }
  // dihedrals a - me - j - b, me < j
  for (unsigned r = nb & ~((2u << me) - 1u); r; r &= r - 1u) {
    const int j = __ffs(r) - 1;
    const unsigned tj = M.type[j], om = row[j];
    const unsigned char* __restrict__ row_j = M.adj + j * 32;
    const unsigned of_j = M.nb[j] & ~(1u << me);
    for (unsigned ra = nb & ~(1u << j); ra; ra &= ra - 1u) {
      const int a = __ffs(ra) - 1;
      const unsigned ta = M.type[a], oa = row[a];
      for (unsigned rb = of_j; rb; rb &= rb - 1u) {
        const int b = __ffs(rb) - 1;
        const unsigned tb = M.type[b], ob = row_j[b];
        if ((ta | oa | ti | om | tj | ob | tb) > 15u) continue;
        const int k = class_of(M.tbl[2], ta | oa << 4 | ti << 8 | om << 12 | tj << 16 | ob << 20 | tb << 24,
                               tb | ob << 4 | tj << 8 | om << 12 | ti << 16 | oa << 20 | ta << 24);
        if (k < 0) continue;
        float v;
        const bool ok = dihedral_value(M.pos[a], M.pos[me], M.pos[j], M.pos[b], v);
        emit(2, k, ok, v);
      }
    }
  }
}

struct Tables {
  const int32_t* cls[3];
  int n[3];
};

// record p into LDS; returns its atom count
__device__ int load_record(Mol& M, const unsigned char* __restrict__ rec, const int32_t* __restrict__ n_atoms, const Tables& T, int64_t p,
                           int lane) {
  const int n = ds_rec::atoms_of(n_atoms, p);
  const unsigned char* __restrict__ mine = rec + p * DS_RECORD_BYTES;
  if (lane < NC) {
#pragma unroll
    for (int kind = 0; kind < 3; ++kind) M.tbl[kind][lane] = lane < T.n[kind] ? T.cls[kind][lane] : -1;
  }
  if (n > 0) ds_rec::load_bonds(M.adj, mine, (1u << n) - 1u, lane);
  if (lane < n) {
    const float* __restrict__ xyz = reinterpret_cast<const float*>(mine + DS_REC_POS) + lane * 3;
    M.pos[lane][0] = (double)xyz[0]; M.pos[lane][1] = (double)xyz[1]; M.pos[lane][2] = (double)xyz[2];
    M.type[lane] = mine[DS_REC_TYPE + lane];
  }
  __syncthreads();
  if (lane < 32) {
    unsigned bonded = 0u;
    if (lane < n)
      for (int j = 0; j < MA; ++j)
        if (M.adj[lane * 32 + j]) bonded |= 1u << j;
    M.nb[lane] = bonded;
  }
  __syncthreads();
  return n;
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int s = 32; s; s >>= 1) v += __shfl_xor(v, s);
  return v;
}

// entries of the lanes below mine
__device__ __forceinline__ int wave_before(int v, int lane) {
  int inc = v;
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const int up = __shfl_up(inc, s);
    if (lane >= s) inc += up;
  }
  return inc - v;
}

__global__ __launch_bounds__(64) void k_geometry_count(const unsigned char* __restrict__ rec, const int32_t* __restrict__ n_atoms, Tables T,
                                                       int32_t* __restrict__ counts, int32_t* __restrict__ skipped) {
  __shared__ Mol M;
  const int64_t p = blockIdx.x;
  const int lane = threadIdx.x;
  const int n = load_record(M, rec, n_atoms, T, p, lane);
  int cnt[3] = {0, 0, 0}, skip = 0;
  Sink none{};
  if (lane < n) walk<false>(M, lane, cnt, skip, none);
  const int c0 = wave_sum(cnt[0]), c1 = wave_sum(cnt[1]), c2 = wave_sum(cnt[2]), sk = wave_sum(skip);
  if (lane == 0) { counts[p * 3] = c0; counts[p * 3 + 1] = c1; counts[p * 3 + 2] = c2; skipped[p] = sk; }
}

__global__ __launch_bounds__(64) void k_geometry_fill(const unsigned char* __restrict__ rec, const int32_t* __restrict__ n_atoms, Tables T,
                                                      const int64_t* __restrict__ offsets, Sink sink) {
  __shared__ Mol M;
  Sink out = sink;
  const int64_t p = blockIdx.x;
  const int lane = threadIdx.x;
  const int n = load_record(M, rec, n_atoms, T, p, lane);
  int cnt[3] = {0, 0, 0}, skip = 0;
  if (lane < n) walk<false>(M, lane, cnt, skip, out);
#pragma unroll
  for (int kind = 0; kind < 3; ++kind) out.at[kind] = offsets[p * 3 + kind] + wave_before(cnt[kind], lane);
  int again[3] = {0, 0, 0};
  if (lane < n) walk<true>(M, lane, again, skip, out);
}

inline bool tables_ok(int32_t a, int32_t b, int32_t c) { return a >= 0 && a <= NC && b >= 0 && b <= NC && c >= 0 && c <= NC; }
const int PRESENT = 0;                                     // stands for a pointer that is not required
inline const void* needed(bool need, const void* p) { return need ? p : &PRESENT; }

}  // namespace

extern "C" int ds_geometry_count_records(const uint8_t* rec, const int32_t* n, int64_t P, const int32_t* bond_cls, int32_t n_bond_cls,
                                         const int32_t* angle_cls, int32_t n_angle_cls, const int32_t* dihedral_cls, int32_t n_dihedral_cls,
                                         int32_t* counts, int32_t* skipped, void* stream) {
  const int go = ds_rec::check_table(tables_ok(n_bond_cls, n_angle_cls, n_dihedral_cls), P, rec, n,
                                     {needed(n_bond_cls > 0, bond_cls), needed(n_angle_cls > 0, angle_cls),
                                      needed(n_dihedral_cls > 0, dihedral_cls), counts, skipped});
  if (go != ds_rec::LAUNCH) return go;
  const Tables T{{bond_cls, angle_cls, dihedral_cls}, {n_bond_cls, n_angle_cls, n_dihedral_cls}};
  hipLaunchKernelGGL(k_geometry_count, dim3((unsigned)P), dim3(64), 0, (hipStream_t)stream, rec, n, T, counts, skipped);
  return DST_CHECK_LAUNCH();
}

extern "C" int ds_geometry_fill_records(const uint8_t* rec, const int32_t* n, int64_t P, const int32_t* bond_cls, int32_t n_bond_cls,
                                        const int32_t* angle_cls, int32_t n_angle_cls, const int32_t* dihedral_cls, int32_t n_dihedral_cls,
                                        int64_t total_bond, int64_t total_angle, int64_t total_dihedral, const int64_t* offsets,
                                        float* bond_value, uint8_t* bond_class, float* angle_value, uint8_t* angle_class,
                                        float* dihedral_value, uint8_t* dihedral_class, void* stream) {
  const bool sizes_ok = tables_ok(n_bond_cls, n_angle_cls, n_dihedral_cls) && total_bond >= 0 && total_angle >= 0 && total_dihedral >= 0;
  const int go = ds_rec::check_table(sizes_ok, P, rec, n,
                                     {needed(n_bond_cls > 0, bond_cls), needed(n_angle_cls > 0, angle_cls),
                                      needed(n_dihedral_cls > 0, dihedral_cls), offsets, needed(total_bond > 0, bond_value),
                                      needed(total_bond > 0, bond_class), needed(total_angle > 0, angle_value),
                                      needed(total_angle > 0, angle_class), needed(total_dihedral > 0, dihedral_value),
                                      needed(total_dihedral > 0, dihedral_class)});
  if (go != ds_rec::LAUNCH) return go;
  const Tables T{{bond_cls, angle_cls, dihedral_cls}, {n_bond_cls, n_angle_cls, n_dihedral_cls}};
  const Sink out{{bond_value, angle_value, dihedral_value}, {bond_class, angle_class, dihedral_class}, {0, 0, 0},
                 {total_bond, total_angle, total_dihedral}};
  hipLaunchKernelGGL(k_geometry_fill, dim3((unsigned)P), dim3(64), 0, (hipStream_t)stream, rec, n, T, offsets, out);
  return DST_CHECK_LAUNCH();
}
