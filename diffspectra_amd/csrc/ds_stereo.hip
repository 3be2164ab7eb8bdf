// diffspectra_amd - stereo-aware molecular identity of the evaluation path: is the generated molecule the ground-truth molecule as a labelled
// graph AND in the spatial arrangement of its four-coordinate centres and double bonds (same stereoisomer, mirror image, another
// stereoisomer, or geometry too flat to tell).  include/diffspectra_stereo.h states every definition (twins, ordinals, the two kinds of
// site, what an isomorphism does to a site, the verdicts); DESIGN.md section 21 has the method, the soundness of the twin rule and the figures.
//
// One wave64 per pair, one wave per workgroup: the generated molecule in lanes 0..28, the ground truth in lanes 32..60, as k_graph_identity
// (ds_graph.hip).  k_stereo_identity calls the pair search of ds_refine.h, where the argument for it stands, and adds two things: the
// initial colour and the leaf's labels also hold the twin ordinal, and the search goes on after a verified leaf, so that it meets every
// ordinal-respecting isomorphism exactly once.  perceive() is the prologue, run per half wave: twins, ordinals and the site bits in fp64, a
// site per lane.  After it the kernel is integers only; no atomics.
//
// Soundness, in the lines the code keeps true: a leaf counts only after ds_refine::verify() has compared every type, charge, ordinal and bond
// byte under an explicit bijection; DSC_DIFFERENT needs an exhausted search without such a leaf; DSC_MIRROR / DSC_STEREOISOMER need an
// exhausted search, so that no same phi was missed; a search the budget stops is DSC_UNDECIDED whatever it had found.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/diffspectra_stereo.h"
#include "ds_records.h"
#include "ds_refine.h"
#include "ds_vec.h"
#include "ds_host.h"   // DST_CHECK_LAUNCH

namespace {

using ds_rec::MA;
constexpr unsigned ALL = ~0u;             // keep mask of ds_rec::load_bonds: every atom (the rows are read up to n only)

__device__ __forceinline__ unsigned half_of(unsigned long long ballot, int side) { return (unsigned)(ballot >> (32 * side)); }

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
  unsigned char positive[64], cis[64], low[64];   // the site bits a leaf is tested against: sign of a centre, cis bit and lowest substituent of an end
  __device__ __forceinline__ const unsigned char* bonds(int side) const { return adj[side]; }
};

struct Site {                             // what a lane knows of its atom after the prologue
  unsigned type, fc, nbr;                 // type byte, charge byte, bit j = bonded to atom j
  int ord, mate, low;                     // ordinal; E/Z: the other end and the lowest substituent (both -1 off-site)
  bool twin, tetra, t_assigned, t_positive, ez, ez_assigned, ez_cis;
  double V;
};

using namespace ds_vec;                   // Vec and its operations: shared with ds_key.hip
__device__ __forceinline__ Vec at(const Geometry& S, int slot) { return {(double)S.pos[slot][0], (double)S.pos[slot][1], (double)S.pos[slot][2]}; }

// The prologue of one molecule per half wave (side = lane >> 5; n = the side's atom count, 0 for a half without a molecule, whose record is
// not touched).  The caller has loaded S.adj[side] and passed the barrier behind it.  Called by the whole wave: it holds barriers.
__device__ __forceinline__ Site perceive(Geometry& S, const unsigned char* __restrict__ mine, int n, int lane, double min_volume, double min_planarity) {
  const int idx = lane & 31, side = lane >> 5, base = side * 32;
  const bool active = idx < n;
  const unsigned char* __restrict__ adj = S.adj[side];
  Site s = {0u, 0u, 0u, 0, -1, -1, false, false, false, false, false, false, false, __builtin_nan("")};
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

  // twins: equal keys.  A leaf's key is (parent, order, type, charge), a bondless atom's (type, charge), every other atom's is its own
  unsigned key = 3u << 29 | (unsigned)lane;
  if (active && deg == 1) {
    const int parent = __ffs((int)nbr) - 1;
    key = 1u << 29 | (unsigned)parent << 24 | (unsigned)adj[idx * 32 + parent] << 16 | s.type << 8 | s.fc;
  } else if (active && deg == 0) {
    key = 2u << 29 | s.type << 8 | s.fc;
  }
  S.key[lane] = key;
  __syncthreads();
  if (active)
    for (int j = 0; j < n; ++j) {
      const bool same = S.key[base + j] == key;
      s.ord += same && j < idx;
      s.twin |= same && j != idx;
    }
  const unsigned twins = half_of(__ballot(s.twin), side);

  // tetrahedral site: four neighbours, none of them a twin (a twin's twins hang on the same atom)
  s.tetra = active && deg == 4 && !(nbr & twins);
  if (s.tetra) {
    const Vec x = at(S, lane);
    bool fin = finite(x);
    unsigned m = nbr;
    auto unit = [&]() {
      const int j = __ffs((int)m) - 1;
      m &= m - 1u;
      const Vec y = at(S, base + j);
      fin &= finite(y);
      const Vec d = y - x;
      return d * (1.0 / sqrt(dot(d, d)));
    };
    const Vec u1 = unit(), u2 = unit(), u3 = unit(), u4 = unit();
    s.V = dot(u1 - u4, cross(u2 - u4, u3 - u4));
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
    const Vec xa = at(S, lane), xb = at(S, base + mate), e = xb - xa;
    const double ee = dot(e, e);
    bool ok = finite(xa) && finite(xb);
    unsigned cis = 0u;
    int k = 0;                             // pair (i-th substituent of a, j-th of b) -> bit i * nt + j
    for (unsigned sm = subs; sm; sm &= sm - 1u)
      for (unsigned tm = mate_subs; tm; tm &= tm - 1u, ++k) {
        const Vec xs = at(S, base + __ffs((int)sm) - 1), xt = at(S, base + __ffs((int)tm) - 1);
        const Vec v = xs - xa, w = xt - xb;
        const Vec p = v - e * (dot(v, e) / ee), q = w - e * (dot(w, e) / ee);
        const double lp = sqrt(dot(p, p)), lq = sqrt(dot(q, q));
        const double c = dot(p, q) / (lp * lq);
        ok &= finite(xs) && finite(xt) && lp > 0.0 && lq > 0.0 && fabs(c) >= min_planarity;
        cis |= (c > 0.0 ? 1u : 0u) << k;
      }
    const int ns = __popc(subs), nt = __popc(mate_subs);
    auto bit = [&](int i, int j) { return (cis >> (i * nt + j)) & 1u; };
    if (ns == 2)
      for (int j = 0; j < nt; ++j) ok &= bit(0, j) != bit(1, j);
    if (nt == 2)
      for (int i = 0; i < ns; ++i) ok &= bit(i, 0) != bit(i, 1);
    res = (ok ? 1u : 0u) | (cis & 1u) << 1;
    S.ezres[lane] = (unsigned char)res;
  }
  __syncthreads();
  if (s.ez && idx > mate) res = S.ezres[base + mate];
  s.ez_assigned = s.ez && (res & 1u);
  s.ez_cis = s.ez_assigned && (res & 2u);
  return s;
}

using ds_refine::Ranked;                  // the joint ranking and the refinement of both molecules at once: ds_refine.h, PAIR = true
using ds_refine::MISMATCH;
using ds_refine::DISCRETE;
using ds_refine::CELLS;
constexpr ds_refine::Block SYNC{};        // one wave per workgroup: the workgroup barrier orders the pair's LDS traffic

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
  int out = DSC_INVALID, used = 0, image = -1;
  int isos = 0, sames = 0, mirrors = 0, tetra_a = 0, ez_a = 0, open_a = 0, open_b = 0;
  if (q.valid) {
    const int ng = q.n_prb(), nr = q.n_ref();
    ds_rec::load_bonds(S.adj[0], q.prb, ALL, lane);
    ds_rec::load_bonds(S.adj[1], q.ref, ALL, lane);
    __syncthreads();
    const Site me = perceive(S, side ? q.ref : q.prb, side ? nr : ng, lane, min_volume, min_planarity);
    const bool ez_low = me.ez && idx < me.mate;             // an E/Z site counts once, at its lower end
    const unsigned centres = half_of(__ballot(me.tetra), 0);
    const unsigned long long open = __ballot((me.tetra && !me.t_assigned) || (ez_low && !me.ez_assigned));
    tetra_a = __popc(centres);
    ez_a = __popc(half_of(__ballot(ez_low), 0));
    open_a = __popc(half_of(open, 0));
    open_b = __popc(half_of(open, 1));
    const bool assigned = open == 0ull;
    out = DSC_DIFFERENT;
    if (ng == nr) {
      const int n = ng;
      const bool active = idx < n;
      S.type[lane] = (unsigned char)me.type;
      S.fc[lane] = (unsigned char)me.fc;
      S.ord[lane] = (unsigned char)me.ord;
      S.positive[lane] = me.t_positive;
      S.cis[lane] = me.ez_cis;
      S.low[lane] = (unsigned char)(me.low & 31);
      __syncthreads();
      // initial colour: (type, charge, ordinal) ranked jointly
      const Ranked first = ds_refine::rank_jointly<true>(S, (unsigned long long)(me.type << 16 | me.fc << 8 | (unsigned)me.ord), n, lane, SYNC);
      int colour = active ? first.colour : 0;
      unsigned long long multi = 0ull;
      int st = __ballot(active && first.eq_g != first.eq_r) ? MISMATCH : ds_refine::refine<true>(S, colour, active, n, lane, multi, SYNC);
      int depth = 0;                                         // open levels: S.stack[0 .. depth-1]
      int first_iso = -1, first_same = -1, first_mirror = -1; // this lane's image under the first isomorphism of each kind
      bool ended = false;                                    // the search stopped for another reason than the budget
      const auto same_label = [](int a, int b) { return S.type[a] == S.type[b] && S.fc[a] == S.fc[b] && S.ord[a] == S.ord[b]; };
      for (int it = 0; it <= max_nodes; ++it) {              // every pass but the last spends one search node
        if (st == DISCRETE && ds_refine::verify(S, colour, active, n, lane, same_label)) {
          const int mine = active && side == 0 ? S.img[idx] : -1;
          if (isos++ == 0) first_iso = mine;
          bool same = false;
          if (assigned) {                                    // the leaf against the site bits, in integers
            bool inverted = false, ez_bad = false;
            if (side == 0 && me.tetra) {                     // B's sign at the image, times the parity of the order of the four images
              unsigned m = me.nbr;
              const int a = S.img[__ffs((int)m) - 1]; m &= m - 1u;
              const int b = S.img[__ffs((int)m) - 1]; m &= m - 1u;
              const int c = S.img[__ffs((int)m) - 1]; m &= m - 1u;
              const int d = S.img[__ffs((int)m) - 1];
              const int odd = ((a > b) + (a > c) + (a > d) + (b > c) + (b > d) + (c > d)) & 1;
              inverted = (int)me.t_positive != (S.positive[32 + mine] ^ odd);
            }
            if (side == 0 && me.ez) {                        // B's cis bit, flipped for every image that is not the lowest substituent of its end
              const int mate = S.img[me.mate];
              const int flips = (S.img[me.low] != S.low[32 + mine]) ^ (S.img[S.low[me.mate]] != S.low[32 + mate]);
              ez_bad = (int)me.ez_cis != (S.cis[32 + mine] ^ flips);
            }
            const unsigned turned = half_of(__ballot(inverted), 0);
            const bool ez_kept = __ballot(ez_bad) == 0ull;
            same = turned == 0u && ez_kept;
            if (same && sames++ == 0) first_same = mine;
            if (centres != 0u && turned == centres && ez_kept && mirrors++ == 0) first_mirror = mine;
          }
          if (!exhaustive && (same || !assigned)) { ended = true; break; }
        }
        if (st == CELLS) {
          if (depth >= MA) break;                            // (cannot happen: every level makes one more generated atom a class of its own)
          ds_refine::open_level(S, depth, colour, active, lane, multi);
        }
        const ds_refine::Try t = ds_refine::next_try(S, depth, colour, active, lane);
        if (t.w < 0) { ended = true; break; }                // nothing left to try anywhere: every isomorphism has been met
        if (used >= max_nodes) break;                        // the budget does not cover this try: undecided
        ++used;
        st = ds_refine::individualise(S, depth, t, colour, active, n, lane, multi);
      }
      out = DSC_UNDECIDED;
      if (ended) {
        if (isos == 0) out = DSC_DIFFERENT;
        else if (!assigned) { out = DSC_UNASSIGNED; image = first_iso; }
        else if (sames) { out = DSC_IDENTICAL; image = first_same; }
        else if (mirrors) { out = DSC_MIRROR; image = first_mirror; }
        else { out = DSC_STEREOISOMER; image = first_iso; }
      }
    }
  }
  if (lane < MA) map[p * MA + lane] = image;                 // -1 unless this lane is a generated atom and the verdict has a map
  if (lane < 3) found[p * 3 + lane] = lane == 0 ? isos : lane == 1 ? sames : mirrors;
  if (lane < 4) sites[p * 4 + lane] = lane == 0 ? tetra_a : lane == 1 ? ez_a : lane == 2 ? open_a : open_b;
  if (lane == 0) {
    verdict[p] = (unsigned char)out;
    nodes[p] = used;
  }
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
                                        (unsigned)__ballot(me.twin)};
#pragma unroll
  for (int k = 0; k < DSC_NUM_MASKS; ++k)
    if (lane == k) masks[p * DSC_NUM_MASKS + k] = (int32_t)(usable ? rows[k] : 0u);
  if (lane < MA) volume[p * MA + lane] = usable && me.tetra ? me.V : __builtin_nan("");
  if (lane == 0) status[p] = (unsigned char)(usable ? DSC_OK : DSC_UNUSABLE);
}

static_assert(DSC_MASK_TETRA_SITE == 0 && DSC_MASK_TETRA_ASSIGNED == 1 && DSC_MASK_TETRA_POSITIVE == 2 && DSC_MASK_EZ_SITE == 3 &&
              DSC_MASK_EZ_ASSIGNED == 4 && DSC_MASK_EZ_CIS == 5 && DSC_MASK_TWIN == 6, "the order of rows[] in k_stereo_sites");
static_assert(DSC_DIFFERENT == DS_GRAPH_DIFFERENT && DSC_IDENTICAL == DS_GRAPH_IDENTICAL && DSC_UNDECIDED == DS_GRAPH_UNDECIDED &&
              DSC_INVALID == DS_GRAPH_INVALID, "the codes 0..3 mean what DS_GRAPH_* mean");

bool thresholds_ok(double min_volume, double min_planarity) { return min_volume >= 0.0 && min_planarity >= 0.0; }   // false for a NaN

}  // namespace

extern "C" int dsc_stereo_identity_records(const uint8_t* prb_rec, const int32_t* prb_n, int64_t P, const uint8_t* ref_rec, const int32_t* ref_n,
                                           int64_t M, const int64_t* ref_index, int32_t max_nodes, double min_volume, double min_planarity,
                                           int32_t exhaustive, uint8_t* verdict, int32_t* nodes, int32_t* found, int32_t* sites, int32_t* map,
                                           void* stream) {
  const bool scalars_ok = max_nodes >= 0 && max_nodes <= DS_GRAPH_MAX_NODES && thresholds_ok(min_volume, min_planarity) &&
                          (exhaustive == 0 || exhaustive == 1);
  const int go = ds_rec::check_pairs(scalars_ok, P, M, prb_rec, prb_n, ref_rec, ref_n, ref_index, {verdict, nodes, found, sites, map});
  if (go != ds_rec::LAUNCH) return go;
  hipLaunchKernelGGL(k_stereo_identity, dim3((unsigned)P), dim3(64), 0, (hipStream_t)stream, prb_rec, prb_n, ref_rec, ref_n, ref_index, M,
                     (int)max_nodes, min_volume, min_planarity, (int)exhaustive, verdict, nodes, found, sites, map);
  return DST_CHECK_LAUNCH();
}

extern "C" int dsc_stereo_sites(const uint8_t* rec, const int32_t* n, int64_t P, double min_volume, double min_planarity, int32_t* masks,
                                double* volume, uint8_t* status, void* stream) {
  const int go = ds_rec::check_table(thresholds_ok(min_volume, min_planarity), P, rec, n, {masks, volume, status});
  if (go != ds_rec::LAUNCH) return go;
  hipLaunchKernelGGL(k_stereo_sites, dim3((unsigned)P), dim3(64), 0, (hipStream_t)stream, rec, n, min_volume, min_planarity, masks, volume, status);
  return DST_CHECK_LAUNCH();
}
