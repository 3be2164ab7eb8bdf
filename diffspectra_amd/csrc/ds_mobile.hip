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
#include "ds_perceive.h"
#include "ds_host.h"   // DST_CHECK_LAUNCH

namespace {

using namespace ds_perceive;

struct Wave {                             // one record's staging area
  unsigned char adj[MA * 32];             // symmetric bond orders over original atom indices, diagonal 0
  unsigned todo[DSM_LEVELS][32];          // [level][donor lane]: the interior atoms still to be tried from the level's last atom
  unsigned short step[DSM_LEVELS][32];    // [level][donor lane]: the atoms v | w << 8 that the extension into this level put on the path
  unsigned single[32];                    // bit j = bonded to atom j by order 1 and atom j is an interior atom
  unsigned found[32];                     // a donor's acceptors
  unsigned char partner[32];              // the other end of an interior atom's double bond
  unsigned char ht[32];                   // normalised hydrogen count
};

struct Found {                            // what the analysis leaves; kept, roots, groups, p, nodes, mobile and status are wave-uniform
  int status;                             // DSM_OK, DSM_UNUSABLE or DSM_UNDECIDED
  bool kept_atom, member;                 // this lane holds a kept atom / a member of a group
  int q_res, ht, group;                   // of this lane's atom; group = -1 for no member
  unsigned kept_nb, kept, comp, roots;    // kept neighbours; kept atoms; the members of this atom's group; the lowest atom of every group
  int groups, p, nodes, mobile;
};

__device__ __forceinline__ Found analyse(Wave& S, const unsigned char* __restrict__ mine, int n, int lane, int max_nodes) {
  const ds_refine::Wave sync{};
  const Atom A = scan(S.adj, mine, n, lane, sync);
  const bool usable = usable_record(A, n), on = usable && A.active;
  const int t = min(A.type, MAX_TYPE);
  const unsigned nb = on ? A.nb : 0u, nb1 = on ? A.nb1 : 0u, nb2 = on ? A.nb2 : 0u, nb3 = on ? A.nb3 : 0u;
  const unsigned me = lane < 32 ? 1u << lane : 0u;

  // 1. the fold
  const unsigned isH = low32(__ballot(on && t == H));
  const unsigned folded = low32(__ballot(plain_hydrogen(on, t, A.raw, nb, isH) && nb1 == nb));
  const unsigned kept = low32(__ballot(on)) & ~folded;
  const bool kept_atom = (kept & me) != 0u;
  const int q = on ? applied_charge(t, A.raw) : 0;
  int ht = kept_atom ? __popc(nb & folded) + max(0, max_valence(t, q) - A.val) : 0;
  const int dbl = __popc(nb2), trp = __popc(nb3);

  // 2. charges, judged on the input
  const unsigned plus = low32(__ballot(kept_atom && q > 0)), minus = low32(__ballot(kept_atom && q < 0));
  const bool paired = (q > 0 && (nb & minus)) || (q < 0 && (nb & plus));
  int q_res = kept_atom ? q : 0, dp = 0;
  if (kept_atom && !paired) {
    if (t == N && q == 1 && ht >= 1) { ht -= 1; q_res = 0; dp = 1; }
    else if ((t == N || t == O) && q == -1) { ht += 1; q_res = 0; dp = -1; }
  }
  const int p = wave_sum(dp);

  // 3. endpoints and interior atoms
  const bool candidate = kept_atom && (t == N || t == O) && q_res == 0 && trp == 0 && dbl <= 1;
  const bool donor = candidate && ht >= 1 && dbl == 0, acceptor = candidate && dbl == 1;
  const unsigned acceptors = low32(__ballot(acceptor));
  const unsigned interior = low32(__ballot(kept_atom && (t == C || t == N) && q_res == 0 && dbl == 1 && trp == 0));
  if (lane < 32) {
    S.single[lane] = nb1 & interior;
    S.partner[lane] = (unsigned char)(nb2 ? __ffs((int)nb2) - 1 : 0);
    S.ht[lane] = (unsigned char)ht;
    S.found[lane] = 0u;
  }
  sync();

  // 4. and 6. the search of this lane's donor: at most max_nodes + 1 extensions, each followed by one pop at the most
  int count = 0;
  if (donor && acceptors) {
    unsigned onpath = me, found = 0u;
    int depth = 0;
    S.todo[0][lane] = nb1 & interior;
    for (int it = 0; it <= 2 * max_nodes + 2; ++it) {
      const unsigned left = S.todo[depth][lane];
      if (!left) {
        if (depth == 0) break;
        const unsigned s = S.step[depth][lane];
        onpath &= ~((1u << (s & 31u)) | (1u << ((s >> 8) & 31u)));
        --depth;
        continue;
      }
      const int v = __ffs((int)left) - 1;
      S.todo[depth][lane] = left & (left - 1u);
      if (++count > max_nodes) break;
      const int w = S.partner[v] & 31;
      const unsigned wbit = 1u << w;
      if (onpath & wbit) continue;
      if (acceptors & wbit) {
        found |= wbit;
        if (found == acceptors) break;
      }
      if ((interior & wbit) && depth + 1 < DSM_LEVELS) {
        const unsigned both = (1u << v) | wbit, next = S.single[w] & ~(onpath | both);
        if (next) {
          ++depth;
          onpath |= both;
          S.todo[depth][lane] = next;
          S.step[depth][lane] = (unsigned short)(v | (w << 8));
        }
      }
    }
    S.found[lane] = found;
  }
  const int nodes = wave_sum(min(count, max_nodes + 1));                          // (29 * (DSM_MAX_NODES + 1) fits an int)
  const bool decided = nodes <= max_nodes;
  sync();

  // 5. groups: ~ made symmetric, then its components
  unsigned comp = 0u;
  if (donor) comp = S.found[lane];
  if (acceptor)
    for (int j = 0; j < n; ++j)
      if ((S.found[j] >> lane) & 1u) comp |= 1u << j;
  if (comp) comp |= me;
  comp = components(comp, n);
  const bool member = usable && decided && comp != 0u;
  const unsigned roots = low32(__ballot(member && (unsigned)(__ffs((int)comp) - 1) == (unsigned)lane));
  const int group = member ? (int)__popc(roots & ((1u << (__ffs((int)comp) - 1)) - 1u)) : -1;
  const int mobile = wave_sum(member ? ht : 0);
  const int status = !usable ? DSM_UNUSABLE : !decided ? DSM_UNDECIDED : DSM_OK;
  return {status, kept_atom, member, q_res, ht, group, nb & kept, kept, comp, roots, (int)__popc(roots), p, nodes, mobile};
}

// the mobile H of the group whose lowest atom is this lane's (asked by the root lanes only)
__device__ __forceinline__ int group_hydrogens(const Wave& S, unsigned comp) {
  int h = 0;
  for (unsigned m = comp; m; m &= m - 1u) h += S.ht[__ffs((int)m) - 1];
  return h;
}

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
static_assert(DSM_MAX_GROUPS == MA / 2 && DSM_LEVELS >= (MA - 1) / 2 + 1, "groups of two atoms at least; a simple path of MA atoms has (MA - 1) / 2 extensions");
static_assert(DS_REC_POS % 4 == 0 && DS_RECORD_BYTES % 4 == 0, "positions and rows as dwords");
static_assert(DSM_GROUP_TYPE > MAX_TYPE && DSM_PROTON_TYPE > DSM_GROUP_TYPE, "normal-form records are outside the alphabet of the analytics");
static_assert(DSM_MAX_NODES <= (0x7fffffff - 2) / 2 && DSM_MAX_NODES < 0x7fffffff / 64, "the search's pass counter and the wave's node sum fit an int");

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
