// diffspectra_amd - mobile-hydrogen (tautomer) and proton-balance analytics on result records: the groups of N and O atoms that share mobile
// hydrogens, the hydrogens fixed on every other atom, the residual charges and the proton balance, and the record rewritten in the normal
// form whose labelled-graph identity is identity at the level of a standard InChI's main layer.  include/diffspectra_mobile.h states every
// definition (the fold, the charge normalisation, donors, acceptors and interior atoms, the simple alternating shift path, the groups, the
// search order and its budget, the normal form); DESIGN.md section 23 has the method and the figures.
//
// One wave64 per record, DSM_WAVES records per workgroup, an atom per lane.  The scan, the fold, the applied charge and Vmax are those of
// ds_perceive.h.  An interior atom has one double bond, so a shift path is a chain of extensions (over a single bond to an interior atom, on
// over that atom's double bond); every donor lane runs the depth-first search over them on its own, with its stack - the extensions still to
// try at every level, and the two atoms a level put on the path - in LDS, because a stack in registers indexed by the depth would go to
// scratch.  The lanes of a wave diverge inside that loop only; every wave works on its own LDS area, so the kernels hold wave barriers only
// and a wave without a record runs through with n = 0 and writes nothing.  Integers only, no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/diffspectra_mobile.h"
#include "ds_mobile.h"      // the analysis of one record: Wave, Found, analyse()
#include "ds_host.h"   // DST_CHECK_LAUNCH

namespace {

using namespace ds_mobile;              // Wave, Found, analyse(), group_hydrogens(): shared with ds_key.hip

__global__ __launch_bounds__(64 * DSM_WAVES) void k_mobile(const unsigned char* __restrict__ rec, const int32_t* __restrict__ n_atoms, int64_t P,
                                                           int max_nodes, unsigned char* __restrict__ fixed_h, signed char* __restrict__ q_res,
                                                           unsigned char* __restrict__ group_of, unsigned char* __restrict__ group_h,
                                                           int32_t* __restrict__ summary, int32_t* __restrict__ nodes,
                                                           unsigned char* __restrict__ status) {
  __shared__ Wave W[DSM_WAVES];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * DSM_WAVES + wave;
  const bool live = p < P;
  const int n = live ? ds_rec::atoms_of(n_atoms, p) : 0;            // a wave without a record passes n = 0 and touches no record
  Wave& S = W[wave];
  const Found r = analyse(S, rec + (live ? p : 0) * DS_RECORD_BYTES, n, lane, max_nodes);
  if (!live) return;
  const bool ok = r.status == DSM_OK;
  if (lane < MA) {
    fixed_h[p * MA + lane] = (unsigned char)(ok && r.kept_atom ? (r.member ? 0 : r.ht) : 0xff);
    q_res[p * MA + lane] = (signed char)(ok ? r.q_res : 0);
    group_of[p * MA + lane] = (unsigned char)(ok && r.member ? r.group : 0xff);
  }
  if (lane < DSM_MAX_GROUPS && (!ok || lane >= r.groups)) group_h[p * DSM_MAX_GROUPS + lane] = 0xff;
  if (ok && r.member && ((r.roots >> lane) & 1u) && r.group < DSM_MAX_GROUPS)
    group_h[p * DSM_MAX_GROUPS + r.group] = (unsigned char)group_hydrogens(S, r.comp);
  if (lane < 4) {
    const int v = lane == 0 ? __popc(r.kept) : lane == 1 ? r.groups : lane == 2 ? r.mobile : r.p;
    summary[p * 4 + lane] = ok ? v : 0;
  }
  if (lane == 0) {
    nodes[p] = ok ? r.nodes : 0;
    status[p] = (unsigned char)r.status;
  }
}

struct Row {                              // the normal-form kernel's staging area: the analysis and one output row
  Wave w;
  alignas(16) unsigned char out[DS_RECORD_BYTES];
};

__global__ __launch_bounds__(64 * DSM_WAVES) void k_mobile_normal(const unsigned char* __restrict__ rec, const int32_t* __restrict__ n_atoms, int64_t P,
                                                                  int max_nodes, unsigned char* __restrict__ out_rec, int32_t* __restrict__ out_n,
                                                                  unsigned char* __restrict__ out_source, unsigned char* __restrict__ status) {
  __shared__ Row W[DSM_WAVES];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * DSM_WAVES + wave;
  const bool live = p < P;
  const int n = live ? ds_rec::atoms_of(n_atoms, p) : 0;
  Wave& S = W[wave].w;
  unsigned char* row = W[wave].out;                                               // bytes and dwords of one array: no __restrict__
  uint32_t* row_words = reinterpret_cast<uint32_t*>(row);
  const unsigned char* __restrict__ mine = rec + (live ? p : 0) * DS_RECORD_BYTES;
  const Found r = analyse(S, mine, n, lane, max_nodes);
  if (!live) return;
  const ds_refine::Wave sync{};
  const unsigned me = lane < 32 ? 1u << lane : 0u;
  const int K = (int)__popc(r.kept), total = K + r.groups + (r.p != 0 ? 1 : 0);
  const int st = r.status != DSM_OK ? r.status : total > MA ? DSM_OVERFLOW : DSM_OK;
  const bool ok = st == DSM_OK;

  for (int w = lane; w < DS_RECORD_BYTES / 4; w += 64) row_words[w] = 0u;
  sync();
  if (ok && r.kept_atom) {                                                        // slot < K <= total <= MA
    const int slot = (int)__popc(r.kept & (me - 1u));
    const uint32_t* __restrict__ words = reinterpret_cast<const uint32_t*>(mine);
    for (int k = 0; k < 3; ++k) row_words[DS_REC_POS / 4 + slot * 3 + k] = words[DS_REC_POS / 4 + lane * 3 + k];
    row[DS_REC_TYPE + slot] = mine[DS_REC_TYPE + lane];
    row[DS_REC_FC + slot] = (unsigned char)((r.member ? 0 : r.ht) + 16 * (r.q_res + 1));
    for (unsigned left = r.kept_nb; left; left &= left - 1u) {
      const int j = __ffs((int)left) - 1;
      row[DS_REC_BOND + slot * MA + (int)__popc(r.kept & ((1u << j) - 1u))] = 1;
    }
    if (r.member) {
      const int g = K + r.group;
      row[DS_REC_BOND + slot * MA + g] = row[DS_REC_BOND + g * MA + slot] = 1;
      if ((r.roots >> lane) & 1u) {
        row[DS_REC_TYPE + g] = (unsigned char)DSM_GROUP_TYPE;
        row[DS_REC_FC + g] = (unsigned char)group_hydrogens(S, r.comp);
      }
    }
  }
  if (ok && r.p != 0 && lane == 0) {
    row[DS_REC_TYPE + total - 1] = (unsigned char)DSM_PROTON_TYPE;
    row[DS_REC_FC + total - 1] = (unsigned char)(signed char)r.p;
  }
  if (lane < MA) {
    // the kept atom of slot `lane`: the lane-th set bit of kept
    unsigned k = r.kept;
    for (int i = 0; i < lane; ++i) k &= k - 1u;
    out_source[p * MA + lane] = (unsigned char)(ok && lane < K ? __ffs((int)k) - 1 : 0xff);
  }
  if (lane == 0) {
    out_n[p] = ok ? total : 0;
    status[p] = (unsigned char)st;
  }
  sync();
  uint32_t* __restrict__ dst = reinterpret_cast<uint32_t*>(out_rec + p * DS_RECORD_BYTES);
  for (int w = lane; w < DS_RECORD_BYTES / 4; w += 64) dst[w] = row_words[w];
}

static_assert(DSM_WAVES >= 1 && 64 * DSM_WAVES <= 1024, "a workgroup of whole waves");
static_assert(DS_REC_POS % 4 == 0 && DS_RECORD_BYTES % 4 == 0, "positions and rows as dwords");
static_assert(DSM_GROUP_TYPE > MAX_TYPE && DSM_PROTON_TYPE > DSM_GROUP_TYPE, "normal-form records are outside the alphabet of the analytics");

}  // namespace

extern "C" int dsm_mobile_records(const uint8_t* rec, const int32_t* n, int64_t P, int32_t max_nodes, uint8_t* fixed_h, int8_t* q_res, uint8_t* group_of,
                                  uint8_t* group_h, int32_t* summary, int32_t* nodes, uint8_t* status, void* stream) {
  const int go = ds_rec::check_table(max_nodes >= 1 && max_nodes <= DSM_MAX_NODES, P, rec, n, {fixed_h, q_res, group_of, group_h, summary, nodes, status});
  if (go != ds_rec::LAUNCH) return go;
  hipLaunchKernelGGL(k_mobile, dim3((unsigned)((P + DSM_WAVES - 1) / DSM_WAVES)), dim3(64 * DSM_WAVES), 0, (hipStream_t)stream, rec, n, P,
                     (int)max_nodes, fixed_h, q_res, group_of, group_h, summary, nodes, status);
  return DST_CHECK_LAUNCH();
}

extern "C" int dsm_normal_records(const uint8_t* rec, const int32_t* n, int64_t P, int32_t max_nodes, uint8_t* out_rec, int32_t* out_n,
                                  uint8_t* out_source, uint8_t* status, void* stream) {
  const int go = ds_rec::check_table(max_nodes >= 1 && max_nodes <= DSM_MAX_NODES, P, rec, n, {out_rec, out_n, out_source, status});
  if (go != ds_rec::LAUNCH) return go;
  if (reinterpret_cast<uintptr_t>(out_rec) & 3) return DS_ERR_ARG;                // rows are stored as dwords
  hipLaunchKernelGGL(k_mobile_normal, dim3((unsigned)((P + DSM_WAVES - 1) / DSM_WAVES)), dim3(64 * DSM_WAVES), 0, (hipStream_t)stream, rec, n, P,
                     (int)max_nodes, out_rec, out_n, out_source, status);
  return DST_CHECK_LAUNCH();
}
