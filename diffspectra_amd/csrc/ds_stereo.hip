// diffspectra_amd - stereo-aware molecular identity of the evaluation path: is the generated molecule the ground-truth molecule as a labelled
// graph AND in the spatial arrangement of its four-coordinate centres and double bonds (same stereoisomer, mirror image, another
// stereoisomer, or geometry too flat to tell).  include/diffspectra_stereo.h states every definition (twins, ordinals, the two kinds of
// site, what an isomorphism does to a site, the verdicts); DESIGN.md section 21 has the method, the soundness of the twin rule and the figures.
//
// One wave64 per pair, one wave per workgroup: the generated molecule in lanes 0..28, the ground truth in lanes 32..60.  ds_sites.h has the
// twin key, the fp64 geometry of a site, the search with its leaf test and the argument for the verdicts.  What this file adds is perceive(),
// the prologue run per half wave on a record as drawn: neighbours, twins, ordinals and the sites, a site per lane, none of them on a
// hydrogen slot.  After it the kernel is integers only; no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/diffspectra_stereo.h"
#include "ds_records.h"
#include "ds_sites.h"
#include "ds_host.h"   // DST_CHECK_LAUNCH

namespace {

using ds_rec::MA;
using ds_sites::half_of;
constexpr unsigned ALL = ~0u;             // keep mask of ds_rec::load_bonds: every atom (the rows are read up to n only)

struct Geometry {                         // what the prologue stages of both molecules (of one, in k_stereo_sites); arrays of 64 are indexed by lane
  unsigned char adj[2][MA * 32];
  float pos[64][3];
  unsigned key[64], subs[64];             // twin key; the substituents of an atom that can be an end of an E/Z site, else 0
  unsigned char ezres[64];                // what the lower end of an E/Z site found: bit 0 assigned, bit 1 cis
};

struct Pair : Geometry {
  unsigned char type[64], fc[64], ord[64];
  unsigned long long sig[64], f[64];      // signatures being ranked; per-atom colour hash of the running round
  unsigned char stack[MA][64];            // the pair search's fields, as ds_refine.h names them
  int cell[MA], atom[MA], cursor[MA];
  unsigned char inv[64], img[32];
  unsigned char flag[64], mate[64], low[64];   // the site bytes a leaf is tested against, as ds_sites.h names them
  __device__ __forceinline__ const unsigned char* bonds(int side) const { return adj[side]; }
};

struct Site {                             // what a lane knows of its atom after the prologue
  unsigned type, fc, nbr;                 // type byte, charge byte, bit j = bonded to atom j
  int ord, mate, low;                     // ordinal; E/Z: the other end and the lowest substituent (0 and NO_LOW off-site)
  bool twin, tetra, t_assigned, t_positive, ez, ez_assigned, ez_cis;
  double V;
};

// The prologue of one molecule per half wave (side = lane >> 5; n = the side's atom count, 0 for a half without a molecule, whose record is
// not touched).  The caller has loaded S.adj[side] and passed the barrier behind it.  Called by the whole wave: it holds barriers.
__device__ __forceinline__ Site perceive(Geometry& S, const unsigned char* __restrict__ mine, int n, int lane, double min_volume, double min_planarity) {
  const int idx = lane & 31, side = lane >> 5, base = side * 32;
  const bool active = idx < n;
  const unsigned char* __restrict__ adj = S.adj[side];
  const auto at = [&S, base](int atom) { return ds_vec::widen(S.pos[base + atom]); };   // positions of the own side
  Site s = {0u, 0u, 0u, 0, 0, ds_sites::NO_LOW, false, false, false, false, false, false, false, __builtin_nan("")};
  if (active) {
    s.type = mine[DS_REC_TYPE + idx];
    s.fc = mine[DS_REC_FC + idx];
    const float* __restrict__ xyz = reinterpret_cast<const float*>(mine + DS_REC_POS) + idx * 3;
    S.pos[lane][0] = xyz[0]; S.pos[lane][1] = xyz[1]; S.pos[lane][2] = xyz[2];
  }
  unsigned nbr = 0u, multiple = 0u;        // bonded by any order / by order >= 2
  if (active)
    for (int j = 0; j < n; ++j) {
      const unsigned b = adj[idx * 32 + j];
      nbr |= (b ? 1u : 0u) << j;
      multiple |= (b >= 2u ? 1u : 0u) << j;
    }
  s.nbr = nbr;
  const int deg = __popc(nbr);

  // twins: equal keys.  A leaf's bond order is part of its key here
  const int parent = __ffs((int)nbr) - 1;
  const unsigned key = ds_sites::twin_key(active ? deg : 2, parent, deg == 1 ? adj[idx * 32 + parent] : 0u, s.type, s.fc, lane);
  S.key[lane] = key;
  __syncthreads();
  if (active) {
    const ds_sites::Twins t = ds_sites::count_twins(S.key + base, key, n, idx);
    s.ord = t.ord;
    s.twin = t.twin;
  }
  const unsigned twins = half_of(__ballot(s.twin), side);

  // tetrahedral site: four neighbours, none of them a twin (a twin's twins hang on the same atom)
  s.tetra = active && deg == 4 && !(nbr & twins);
  if (s.tetra) {
    bool fin;
    s.V = ds_sites::tetra_volume(at, idx, nbr, 0, fin);
    s.t_assigned = fin && fabs(s.V) >= min_volume;          // a V that is not a number is below every threshold
    s.t_positive = s.t_assigned && s.V > 0.0;
  }

  // E/Z site: one bond of order >= 2, of order 2, one or two substituents and no twins among them - at both ends
  const int mate = multiple ? __ffs((int)multiple) - 1 : 0;
  const bool end_ok = active && __popc(multiple) == 1 && adj[idx * 32 + mate] == 2 && (deg == 2 || deg == 3) && !(nbr & ~(1u << mate) & twins);
  const unsigned subs = end_ok ? nbr & ~(1u << mate) : 0u;
  S.subs[lane] = subs;
  __syncthreads();
  const unsigned mate_subs = end_ok ? S.subs[base + mate] : 0u;
  s.ez = end_ok && mate_subs != 0u;
  unsigned res = 0u;
  if (s.ez) { s.mate = mate; s.low = __ffs((int)subs) - 1; }
  if (s.ez && idx < mate) {               // the lower end works the site out for both
    res = ds_sites::ez_result(at, idx, mate, subs, mate_subs, 0, 0, min_planarity);
    S.ezres[lane] = (unsigned char)res;
  }
  __syncthreads();
  if (s.ez && idx > mate) res = S.ezres[base + mate];
  s.ez_assigned = s.ez && (res & 1u);
  s.ez_cis = s.ez_assigned && (res & 2u);
  return s;
}

__global__ __launch_bounds__(64) void k_stereo_identity(const unsigned char* __restrict__ prb_rec, const int32_t* __restrict__ prb_n,
                                                        const unsigned char* __restrict__ ref_rec, const int32_t* __restrict__ ref_n,
                                                        const int64_t* __restrict__ ref_index, int64_t M, int max_nodes, double min_volume,
                                                        double min_planarity, int exhaustive, unsigned char* __restrict__ verdict,
                                                        int32_t* __restrict__ nodes, int32_t* __restrict__ found, int32_t* __restrict__ sites,
                                                        int32_t* __restrict__ map) {
  __shared__ Pair S;
  const int64_t p = blockIdx.x;
  const int lane = threadIdx.x, idx = lane & 31, side = lane >> 5;
  const ds_rec::Pair q = ds_rec::pair_of(p, prb_rec, prb_n, ref_rec, ref_n, ref_index, M);
  ds_sites::Found r = {DSC_INVALID, -1, 0, 0, 0, 0};
  ds_sites::Census c = {0u, false, 0, 0, 0, 0};
  if (q.valid) {
    const int ng = q.n_prb(), nr = q.n_ref();
    ds_rec::load_bonds(S.adj[0], q.prb, ALL, lane);
    ds_rec::load_bonds(S.adj[1], q.ref, ALL, lane);
    __syncthreads();
    const Site me = perceive(S, side ? q.ref : q.prb, side ? nr : ng, lane, min_volume, min_planarity);
    const bool ez_low = me.ez && idx < me.mate;             // an E/Z site counts once, at its lower end
    c = ds_sites::census(me.tetra, ez_low, (me.tetra && !me.t_assigned) || (ez_low && !me.ez_assigned));
    r.out = DSC_DIFFERENT;
    if (ng == nr) {
      const ds_sites::Node node = {me.type, me.fc, me.ord, me.nbr, me.tetra ? (unsigned)DSI_KIND_CENTRE : me.ez ? DSI_KIND_END : DSI_KIND_NONE,
                                   me.t_positive || me.ez_cis, false, me.mate, me.low};
      r = ds_sites::search(S, node, ng, lane, c.assigned, c.centres, max_nodes, exhaustive);
    }
  }
  ds_sites::write_out(p, lane, r, c, verdict, nodes, found, sites, map);
}

// the prologue on its own: one record per wave, lanes 32..63 hold no molecule
__global__ __launch_bounds__(64) void k_stereo_sites(const unsigned char* __restrict__ rec, const int32_t* __restrict__ n_atoms, double min_volume,
                                                     double min_planarity, int32_t* __restrict__ masks, double* __restrict__ volume,
                                                     unsigned char* __restrict__ status) {
  __shared__ Geometry S;
  const int64_t p = blockIdx.x;
  const int lane = threadIdx.x;
  const int n = ds_rec::atoms_of(n_atoms, p);
  const unsigned char* __restrict__ mine = rec + p * DS_RECORD_BYTES;
  ds_rec::load_bonds(S.adj[0], mine, ALL, lane);
  __syncthreads();
  const Site me = perceive(S, mine, lane < 32 ? n : 0, lane, min_volume, min_planarity);
  bool bad = false;                                          // the unusable rule of diffspectra_valence.h
  if (lane < n) {
    bad = me.type > 4u;
    for (int j = 0; j < n; ++j) bad |= S.adj[0][lane * 32 + j] > 3;
  }
  const bool usable = n > 0 && __ballot(bad) == 0ull;
  const unsigned rows[DSC_NUM_MASKS] = {(unsigned)__ballot(me.tetra), (unsigned)__ballot(me.t_assigned), (unsigned)__ballot(me.t_positive),
                                        (unsigned)__ballot(me.ez), (unsigned)__ballot(me.ez_assigned), (unsigned)__ballot(me.ez_cis),
                                        (unsigned)__ballot(me.twin)};   // in the order of DSC_MASK_* (asserted in ds_sites.h)
#pragma unroll
  for (int k = 0; k < DSC_NUM_MASKS; ++k)
    if (lane == k) masks[p * DSC_NUM_MASKS + k] = (int32_t)(usable ? rows[k] : 0u);
  if (lane < MA) volume[p * MA + lane] = usable && me.tetra ? me.V : __builtin_nan("");
  if (lane == 0) status[p] = (unsigned char)(usable ? DSC_OK : DSC_UNUSABLE);
}

static_assert(DSC_DIFFERENT == DS_GRAPH_DIFFERENT && DSC_IDENTICAL == DS_GRAPH_IDENTICAL && DSC_UNDECIDED == DS_GRAPH_UNDECIDED &&
              DSC_INVALID == DS_GRAPH_INVALID, "the codes 0..3 mean what DS_GRAPH_* mean");

}  // namespace

extern "C" int dsc_stereo_identity_records(const uint8_t* prb_rec, const int32_t* prb_n, int64_t P, const uint8_t* ref_rec, const int32_t* ref_n,
                                           int64_t M, const int64_t* ref_index, int32_t max_nodes, double min_volume, double min_planarity,
                                           int32_t exhaustive, uint8_t* verdict, int32_t* nodes, int32_t* found, int32_t* sites, int32_t* map,
                                           void* stream) {
  const bool scalars_ok = max_nodes >= 0 && max_nodes <= DS_GRAPH_MAX_NODES && ds_sites::thresholds_ok(min_volume, min_planarity) &&
                          (exhaustive == 0 || exhaustive == 1);
  const int go = ds_rec::check_pairs(scalars_ok, P, M, prb_rec, prb_n, ref_rec, ref_n, ref_index, {verdict, nodes, found, sites, map});
  if (go != ds_rec::LAUNCH) return go;
  hipLaunchKernelGGL(k_stereo_identity, dim3((unsigned)P), dim3(64), 0, (hipStream_t)stream, prb_rec, prb_n, ref_rec, ref_n, ref_index, M,
                     (int)max_nodes, min_volume, min_planarity, (int)exhaustive, verdict, nodes, found, sites, map);
  return DST_CHECK_LAUNCH();
}

extern "C" int dsc_stereo_sites(const uint8_t* rec, const int32_t* n, int64_t P, double min_volume, double min_planarity, int32_t* masks,
                                double* volume, uint8_t* status, void* stream) {
  const int go = ds_rec::check_table(ds_sites::thresholds_ok(min_volume, min_planarity), P, rec, n, {masks, volume, status});
  if (go != ds_rec::LAUNCH) return go;
  hipLaunchKernelGGL(k_stereo_sites, dim3((unsigned)P), dim3(64), 0, (hipStream_t)stream, rec, n, min_volume, min_planarity, masks, volume, status);
  return DST_CHECK_LAUNCH();
}
