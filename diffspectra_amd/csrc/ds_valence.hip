// diffspectra_amd - valence analytics on result records: valences, 2-D / 3-D stability, validity, fragments and the fragment extractor
// behind the reference's "Metric-3D" and "Metric-2D" lines.  include/diffspectra_valence.h states every definition (bond orders from the
// record or from the distances, the stability tables, the applied-charge rule, the restated RDKit valence check, the fragment tie rule);
// DESIGN.md section 16 has the figures.
//
// One wave64 per record, DSV_WAVES records per workgroup, an atom per lane.  LDS holds the bond matrix of ds_rec::load_bonds (and, for the
// extractor, three 32-byte tables: type, charge to write, original atom of every kept rank); everything else lives in registers: an atom's
// neighbours are a 29-bit mask, and the components grow by ORing the masks of the atoms reached so far, read with wave shuffles.  No
// atomics, no early exit: a wave whose record lies beyond P takes part in the workgroup's barriers and writes nothing.  From ds_perceive.h:
// the record scan, applied_charge and max_valence, the component doubling, the wave maximum.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/diffspectra_valence.h"
#include "ds_perceive.h"
#include "ds_host.h"   // DST_CHECK_LAUNCH

namespace {

using namespace ds_perceive;
constexpr int REC_WORDS = DS_RECORD_BYTES / 4;

// allowed_fc_bonds of the header as bit sets over the valences 0..4: [element][charge + 1]; a charge outside -1..+1 reads the entry for 0,
// and so does F+, which is no key of the reference's table
static __constant__ unsigned char c_stable_2d[5][3] = {{0x01, 0x02, 0x01}, {0x08, 0x18, 0x08}, {0x04, 0x0c, 0x1c}, {0x02, 0x04, 0x08}, {0x01, 0x02, 0x02}};

struct Wave {                             // one record's staging area
  unsigned char adj[MA * 32];             // symmetric bond orders over original atom indices, diagonal 0
  unsigned char type[32], fc[32], src[32];
};

// The record as ds_perceive::scan reads it, or, with the bonds from the distances, the same with the orders of ds_bonds::order_of in S.adj and
// no charges.  Holds the one workgroup barrier between writing and reading S.adj; bonds_from is the same for the whole launch, so every wave
// reaches it.
__device__ __forceinline__ Atom read_atoms(Wave& S, const unsigned char* __restrict__ mine, int n, int bonds_from, int lane) {
  if (bonds_from == DSV_BONDS_RECORD) return scan(S.adj, mine, n, lane, ds_refine::Block{});
  Atom A = {lane < n, false, 0, 0, 0, 0u, 0u, 0u, 0u};
  if (A.active) A.type = mine[DS_REC_TYPE + lane];
  const int t = min(A.type, MAX_TYPE);
  const float* __restrict__ xyz = reinterpret_cast<const float*>(mine + DS_REC_POS);
  float px = 0.0f, py = 0.0f, pz = 0.0f;
  if (A.active) { px = xyz[lane * 3]; py = xyz[lane * 3 + 1]; pz = xyz[lane * 3 + 2]; }
  for (int j = 0; j < n; ++j) {           // every lane takes part in the shuffles
    const float qx = __shfl(px, j, 64), qy = __shfl(py, j, 64), qz = __shfl(pz, j, 64);
    const int tj = __shfl(t, j, 64);
    int order = 0;
    if (A.active && j != lane) order = ds_bonds::order_of(t, tj, ds_bonds::scaled_distance(px - qx, py - qy, pz - qz));
    A.val += order;
    A.nb |= (order ? 1u : 0u) << j;
    if (A.active) S.adj[lane * 32 + j] = (unsigned char)order;
  }
  __syncthreads();
  A.bad = A.type > MAX_TYPE;
  return A;
}

__global__ __launch_bounds__(64 * DSV_WAVES) void k_valence(const unsigned char* __restrict__ rec, const int32_t* __restrict__ n_atoms, int64_t P,
                                                            int bonds_from, unsigned char* __restrict__ valence, int32_t* __restrict__ stable_mask,
                                                            int32_t* __restrict__ valid_mask, int32_t* __restrict__ summary,
                                                            int32_t* __restrict__ largest_mask, unsigned char* __restrict__ status) {
  __shared__ Wave S[DSV_WAVES];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * DSV_WAVES + wave;
  const bool live = p < P;
  const int n = live ? ds_rec::atoms_of(n_atoms, p) : 0;
  const Atom A = read_atoms(S[wave], rec + (live ? p : 0) * DS_RECORD_BYTES, n, bonds_from, lane);
  const int t = min(A.type, MAX_TYPE);         // a table index whatever the byte; a type above 4 makes the record unusable

  bool stable, valid;
  if (bonds_from == DSV_BONDS_RECORD) {
    const int key = A.raw >= -1 && A.raw <= 1 ? A.raw + 1 : 1;
    stable = A.val <= 4 && ((c_stable_2d[t][key] >> A.val) & 1);
  } else {
    stable = A.val == ds_bonds::c_valence[t];
  }
  valid = A.val <= max_valence(t, applied_charge(t, A.raw));
  const bool usable = usable_record(A, n), on = usable && A.active;
  const unsigned stable_bits = (unsigned)__ballot(on && stable), valid_bits = (unsigned)__ballot(on && valid);

  const unsigned comp = components(on ? (A.nb | (1u << (lane & 31))) : 0u, n);
  const int lowest = __ffs((int)comp) - 1;                                     // -1 for a lane without an atom
  const int fragments = __popcll(__ballot(on && lowest == lane));
  const int best = wave_max(on ? (__popc(comp) << 5) | (31 - lowest) : 0);     // most atoms first, then the lowest first atom
  const unsigned largest = best ? (unsigned)uniform_i(__shfl((int)comp, 31 - (best & 31), 64)) : 0u;

  if (live) {
    if (lane < MA) valence[p * MA + lane] = (unsigned char)(on ? A.val : 0);
    if (lane < 4) {
      const int v = lane == 0 ? n : lane == 1 ? __popc(stable_bits) : lane == 2 ? fragments : best >> 5;
      summary[p * 4 + lane] = usable ? v : 0;
    }
    if (lane == 0) {
      stable_mask[p] = (int32_t)stable_bits;
      valid_mask[p] = (int32_t)valid_bits;
      largest_mask[p] = (int32_t)largest;
      status[p] = (unsigned char)(usable ? DSV_OK : DSV_UNUSABLE);
    }
  }
}

__global__ __launch_bounds__(64 * DSV_WAVES) void k_fragment(const unsigned char* __restrict__ rec, const int32_t* __restrict__ n_atoms, int64_t P,
                                                             int bonds_from, const int32_t* __restrict__ keep, int charge_rule,
                                                             unsigned char* __restrict__ out_rec, int32_t* __restrict__ out_n) {
  __shared__ Wave S[DSV_WAVES];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * DSV_WAVES + wave;
  const bool live = p < P;
  const int n = live ? ds_rec::atoms_of(n_atoms, p) : 0;
  const unsigned char* __restrict__ mine = rec + (live ? p : 0) * DS_RECORD_BYTES;
  Wave& W = S[wave];
  const Atom A = read_atoms(W, mine, n, bonds_from, lane);
  const unsigned kept = usable_record(A, n) ? (unsigned)keep[p] & ((1u << n) - 1u) : 0u;  // n <= 29
  const int m = __popc(kept);
  if (lane < 32) {
    W.type[lane] = (unsigned char)(A.active ? A.type : 0);
    W.fc[lane] = (unsigned char)(charge_rule ? applied_charge(min(A.type, MAX_TYPE), A.raw) : A.raw);   // both 0 with the orders from the distances
    if ((kept >> lane) & 1u) W.src[__popc(kept & ((1u << lane) - 1u))] = (unsigned char)lane;
  }
  __syncthreads();
  if (!live) return;                                                           // the last barrier is behind
  const uint32_t* __restrict__ in = reinterpret_cast<const uint32_t*>(mine);
  uint32_t* __restrict__ out = reinterpret_cast<uint32_t*>(out_rec + p * DS_RECORD_BYTES);
  for (int w = lane; w < REC_WORDS; w += 64) {                                 // the whole record, a dword at a time
    uint32_t v = 0u;
    if (w < DS_REC_TYPE / 4) {                                                 // fp32 coordinate w % 3 of rank w / 3
      const int r = w / 3;
      if (r < m) v = in[W.src[r] * 3 + (w - r * 3)];
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int b = w * 4 + k;
        unsigned byte = 0u;
        if (b < DS_REC_FC) {
          if (b - DS_REC_TYPE < m) byte = W.type[W.src[b - DS_REC_TYPE]];
        } else if (b < DS_REC_BOND) {
          if (b - DS_REC_FC < m) byte = W.fc[W.src[b - DS_REC_FC]];
        } else if (b < DS_REC_BOND_END) {
          const int i = (b - DS_REC_BOND) / MA, j = (b - DS_REC_BOND) - i * MA;
          if (i < m && j < m) byte = W.adj[W.src[i] * 32 + W.src[j]];
        }
        v |= byte << (8 * k);
      }
    }
    out[w] = v;
  }
  if (lane == 0) out_n[p] = m;
}

static_assert(DS_REC_TYPE % 4 == 0, "the positions end on a dword");
static_assert(DSV_WAVES >= 1 && 64 * DSV_WAVES <= 1024, "a workgroup of whole waves");

bool mode_ok(int32_t v) { return v == 0 || v == 1; }

}  // namespace

extern "C" int dsv_valence_records(const uint8_t* rec, const int32_t* n, int64_t P, int32_t bonds_from, uint8_t* valence, int32_t* stable_mask,
                                   int32_t* valid_mask, int32_t* summary, int32_t* largest_mask, uint8_t* status, void* stream) {
  const int go = ds_rec::check_table(mode_ok(bonds_from), P, rec, n, {valence, stable_mask, valid_mask, summary, largest_mask, status});
  if (go != ds_rec::LAUNCH) return go;
  hipLaunchKernelGGL(k_valence, dim3((unsigned)((P + DSV_WAVES - 1) / DSV_WAVES)), dim3(64 * DSV_WAVES), 0, (hipStream_t)stream, rec, n, P,
                     (int)bonds_from, valence, stable_mask, valid_mask, summary, largest_mask, status);
  return DST_CHECK_LAUNCH();
}

extern "C" int dsv_fragment_records(const uint8_t* rec, const int32_t* n, int64_t P, int32_t bonds_from, const int32_t* keep, int32_t charge_rule,
                                    uint8_t* out_rec, int32_t* out_n, void* stream) {
  const int go = ds_rec::check_table(mode_ok(bonds_from) && mode_ok(charge_rule), P, rec, n, {keep, out_rec, out_n});
  if (go != ds_rec::LAUNCH) return go;
  if (reinterpret_cast<uintptr_t>(out_rec) & 3) return DS_ERR_ARG;                // written as dwords
  hipLaunchKernelGGL(k_fragment, dim3((unsigned)((P + DSV_WAVES - 1) / DSV_WAVES)), dim3(64 * DSV_WAVES), 0, (hipStream_t)stream, rec, n, P,
                     (int)bonds_from, keep, (int)charge_rule, out_rec, out_n);
  return DST_CHECK_LAUNCH();
}
