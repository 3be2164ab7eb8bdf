// diffspectra_amd - key-level molecular identity of the evaluation path: is the generated molecule the ground-truth molecule up to mobile
// hydrogens, acid / base forms and Kekule drawings AND in the spatial arrangement of its centres and double bonds - the two layers of the
// InChIKey comparison behind the reference's Top-1, at once.  include/diffspectra_key.h states every definition (the sites at the normalised
// level, the hydrogen slot, the excluded atoms, the bonds on shift paths, what an isomorphism of normal forms does to a site); DESIGN.md
// section 25 has the method and the figures.  All of it restates InChI as remembered and is unpinned against it.
//
// ds_sites.h has the twin key, the fp64 geometry of a site, the search with its leaf test and the argument for the verdicts.  This file adds:
//
// k_key_sites: one wave64 per ORIGINAL record, DSM_WAVES records per workgroup, an atom per lane, wave barriers only.  The mobile-hydrogen
// analysis is that of ds_mobile.h; behind it every donor lane runs the same depth-first search once more without its early stop, on the same
// LDS stack ([level][lane]: a register array indexed by the depth would go to scratch), and marks the double bonds of every path that ends on
// an acceptor.  Then twins, the hydrogen slot and the sites, a site per lane, in original indices; the outputs are written in normal-form
// numbering (the rank of the atom among the kept atoms).
//
// k_key_identity: one wave64 per pair of NORMAL-FORM records, one wave per workgroup, as k_stereo_identity (ds_stereo.hip).  Its prologue
// takes twins and ordinals from the normal form and the sites from the rows, and drops a row that contradicts its record.  No atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/diffspectra_key.h"
#include "ds_mobile.h"
#include "ds_sites.h"
#include "ds_host.h"   // DST_CHECK_LAUNCH

namespace {

using namespace ds_perceive;
using ds_sites::half_of;
using ds_sites::HSLOT;
using ds_sites::NO_LOW;

// ------------------------------------------------------------------------------------------------------------------------ the sites

struct Sites {                            // one record's staging area
  ds_mobile::Wave w;
  float pos[32][3];
  unsigned any[32];                       // neighbours by any order, over all atoms: what ring_bond() walks
  unsigned key[32], subs[32];             // twin key; the substituent word of an atom that can be an end of an E/Z site, else 0
  unsigned char hatom[32];                // the folded hydrogen behind an atom's hydrogen slot
  unsigned char ezres[32];                // what the lower end of an E/Z site found: bit 0 assigned, bit 1 cis
  unsigned char row[32][2];               // the output row, in normal-form numbering
  double vol[32];
};

__global__ __launch_bounds__(64 * DSM_WAVES) void k_key_sites(const unsigned char* __restrict__ rec, const int32_t* __restrict__ n_atoms, int64_t P,
                                                              int max_nodes, double min_volume, double min_planarity,
                                                              unsigned char* __restrict__ site, int32_t* __restrict__ masks,
                                                              double* __restrict__ volume, int32_t* __restrict__ nodes,
                                                              unsigned char* __restrict__ status) {
  __shared__ Sites W[DSM_WAVES];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * DSM_WAVES + wave;
  const bool live = p < P;
  const int n = live ? ds_rec::atoms_of(n_atoms, p) : 0;            // a wave without a record passes n = 0 and touches no record
  Sites& S = W[wave];
  const unsigned char* __restrict__ mine = rec + (live ? p : 0) * DS_RECORD_BYTES;
  const ds_mobile::Found r = ds_mobile::analyse(S.w, mine, n, lane, max_nodes);
  if (!live) return;
  const ds_refine::Wave sync{};
  const unsigned me = lane < 32 ? 1u << lane : 0u;
  const bool in = lane < n;

  if (in) {
    const float* __restrict__ xyz = reinterpret_cast<const float*>(mine + DS_REC_POS) + lane * 3;
    S.pos[lane][0] = xyz[0]; S.pos[lane][1] = xyz[1]; S.pos[lane][2] = xyz[2];
  }
  if (lane < 32) {
    S.any[lane] = r.nb;
    S.row[lane][0] = 0; S.row[lane][1] = DSI_NO_PARTNER;
    S.vol[lane] = 0.0;
  }

  // every shift path: the search of ds_mobile::analyse without its early stop, on the same stack; marked = the interior atoms v whose double
  // bond lies on a path that reached an acceptor (an interior atom has one double bond, so v names the bond)
  int count = 0;
  unsigned marked = 0u;
  if (r.status == DSM_OK && r.donor && r.acceptors) {
    unsigned onpath = me, vpath = 0u;
    int depth = 0;
    S.w.todo[0][lane] = S.w.single[lane];
    for (int it = 0; it <= 2 * max_nodes + 2; ++it) {
      const unsigned left = S.w.todo[depth][lane];
      if (!left) {
        if (depth == 0) break;
        const unsigned s = S.w.step[depth][lane];
        onpath &= ~((1u << (s & 31u)) | (1u << ((s >> 8) & 31u)));
        vpath &= ~(1u << (s & 31u));
        --depth;
        continue;
      }
      const int v = __ffs((int)left) - 1;
      S.w.todo[depth][lane] = left & (left - 1u);
      if (++count > max_nodes) break;
      const int w = S.w.partner[v] & 31;
      const unsigned wbit = 1u << w;
      if (onpath & wbit) continue;
      if (r.acceptors & wbit) marked |= vpath | (1u << v);
      if ((r.interior & wbit) && depth + 1 < DSM_LEVELS) {
        const unsigned both = (1u << v) | wbit, next = S.w.single[w] & ~(onpath | both);
        if (next) {
          ++depth;
          onpath |= both;
          vpath |= 1u << v;
          S.w.todo[depth][lane] = next;
          S.w.step[depth][lane] = (unsigned short)(v | (w << 8));
        }
      }
    }
  }
  const int used = wave_sum(min(count, max_nodes + 1));
  const unsigned on_path = wave_or(marked);
  const int K = (int)__popc(r.kept), total = K + r.groups + (r.p != 0 ? 1 : 0);
  const int st = r.status != DSM_OK ? r.status : used > max_nodes ? DSM_UNDECIDED : total > MA ? DSM_OVERFLOW : DSM_OK;
  const bool ok = st == DSM_OK;
  const bool kept_atom = ok && r.kept_atom;
  sync();

  // the original double bonds of this atom that lie on a shift path / are ring bonds (their other ends are kept atoms)
  const unsigned nb2 = kept_atom ? r.nb2 : 0u;
  const unsigned mobile_nb = (((on_path >> (lane & 31)) & 1u) ? nb2 : 0u) | (nb2 & on_path);
  unsigned ring_nb = 0u;
  for (unsigned left = nb2; left; left &= left - 1u) {
    const unsigned goal = left & (0u - left);
    if (ring_bond(S.any, me, r.nb, goal)) ring_nb |= goal;
  }

  // twins on the normal form: a member's bond to its group node counts, and no bond has an order.  Only a kept atom that is no member can
  // have another atom's key, so the count may run over all n
  const bool excluded = r.member || r.moved;
  const unsigned charge = (unsigned)((r.member ? 0 : r.ht) + 16 * (r.q_res + 1)) & 255u;
  const int degree = (int)__popc(r.kept_nb) + (r.member ? 1 : 0);
  const unsigned key = ds_sites::twin_key(kept_atom && !r.member ? degree : 2, __ffs((int)r.kept_nb) - 1, 0u, (unsigned)mine[DS_REC_TYPE + (in ? lane : 0)], charge, lane);
  if (lane < 32) S.key[lane] = key;
  sync();
  const bool twin = kept_atom && ds_sites::count_twins(S.key, key, n, lane).twin;
  const unsigned twins = low32(__ballot(twin));

  // the hydrogen slot
  const unsigned own_h = r.nb & r.folded;
  const bool hslot = kept_atom && !excluded && r.ht == 1 && __popc(own_h) == 1;
  if (lane < 32) S.hatom[lane] = (unsigned char)(hslot ? __ffs((int)own_h) - 1 : 0);

  const auto at = [&S](int atom) { return ds_vec::widen(S.pos[atom]); };
  // tetrahedral site: kept neighbours + hydrogen slot = 4, no twins among them
  const bool tetra = kept_atom && !excluded && (int)__popc(r.kept_nb) + (hslot ? 1 : 0) == 4 && !(r.kept_nb & twins);
  double V = 0.0;
  bool t_assigned = false;
  if (tetra) {                            // the kept neighbours in ascending index, the hydrogen slot last
    bool fin;
    V = ds_sites::tetra_volume(at, lane, r.kept_nb, __ffs((int)own_h) - 1, fin);
    t_assigned = fin && fabs(V) >= min_volume;              // a V that is not a number is below every threshold
  }
  const bool t_positive = t_assigned && V > 0.0;

  // E/Z site: one bond of order >= 2, of order 2, neither on a shift path nor in a ring, one or two substituents and no twins among them
  const unsigned multiple = kept_atom ? r.nb2 | r.nb3 : 0u;
  const int mate = multiple ? __ffs((int)multiple) - 1 : 0;
  const unsigned kept_subs = r.kept_nb & ~(1u << mate);
  const int n_subs = (int)__popc(kept_subs) + (hslot ? 1 : 0);
  const bool end_ok = kept_atom && !excluded && __popc(multiple) == 1 && nb2 == multiple && !((mobile_nb | ring_nb) & multiple) &&
                      (n_subs == 1 || n_subs == 2) && !(kept_subs & twins);
  const unsigned subs = end_ok ? kept_subs | (hslot ? HSLOT : 0u) : 0u;
  if (lane < 32) S.subs[lane] = subs;
  sync();
  const unsigned mate_subs = end_ok ? S.subs[mate] : 0u;
  const bool ez = end_ok && mate_subs != 0u;
  unsigned res = 0u;
  if (ez && lane < mate) {                // the lower end works the site out for both
    res = ds_sites::ez_result(at, lane, mate, subs, mate_subs, S.hatom[lane], S.hatom[mate], min_planarity);
    S.ezres[lane] = (unsigned char)res;
  }
  sync();
  if (ez && lane > mate) res = S.ezres[mate];
  const bool ez_assigned = ez && (res & 1u), ez_cis = ez_assigned && (res & 2u);

  // the row, in normal-form numbering: a kept atom's index is its rank among the kept atoms
  const int slot = (int)__popc(r.kept & (me - 1u));
  const unsigned at_slot = kept_atom ? 1u << slot : 0u;
  if (kept_atom) {
    const unsigned kind = tetra ? DSI_KIND_CENTRE : ez ? DSI_KIND_END : DSI_KIND_NONE;
    S.row[slot][0] = (unsigned char)(kind | (t_assigned || ez_assigned ? DSI_FLAG_ASSIGNED : 0) | (t_positive || ez_cis ? DSI_FLAG_SIGN : 0) |
                                     (hslot ? DSI_FLAG_HSLOT : 0));
    if (ez) S.row[slot][1] = (unsigned char)__popc(r.kept & ((1u << mate) - 1u));
    if (tetra) S.vol[slot] = V;
  }
  const bool flags[DSI_NUM_MASKS] = {tetra, t_assigned, t_positive, ez, ez_assigned, ez_cis, twin, mobile_nb != 0u, ring_nb != 0u};
#pragma unroll
  for (int k = 0; k < DSI_NUM_MASKS; ++k) {
    const unsigned m = wave_or(flags[k] ? at_slot : 0u);
    if (lane == k) masks[p * DSI_NUM_MASKS + k] = (int32_t)m;
  }
  sync();
  if (lane < MA) {
    site[p * DSI_SITE_BYTES + lane * 2] = S.row[lane][0];
    site[p * DSI_SITE_BYTES + lane * 2 + 1] = S.row[lane][1];
    volume[p * MA + lane] = S.vol[lane];
  }
  if (lane == 0) {
    nodes[p] = ok ? used : 0;
    status[p] = (unsigned char)st;
  }
}

// ------------------------------------------------------------------------------------------------------------------------ the pairs

struct Pair {                             // arrays of 64 are indexed by lane
  unsigned char adj[2][MA * 32];
  unsigned key[64];
  unsigned char type[64], fc[64], ord[64];
  unsigned long long sig[64], f[64];      // signatures being ranked; per-atom colour hash of the running round
  unsigned char stack[MA][64];            // the pair search's fields, as ds_refine.h names them
  int cell[MA], atom[MA], cursor[MA];
  unsigned char inv[64], img[32];
  unsigned char flag[64], mate[64], low[64];   // the site rows a leaf is tested against, and the lowest kept substituent of an end (NO_LOW: none)
  __device__ __forceinline__ const unsigned char* bonds(int side) const { return adj[side]; }
};

__global__ __launch_bounds__(64) void k_key_identity(const unsigned char* __restrict__ prb_rec, const int32_t* __restrict__ prb_n,
                                                     const unsigned char* __restrict__ ref_rec, const int32_t* __restrict__ ref_n,
                                                     const int64_t* __restrict__ ref_index, int64_t M, const unsigned char* __restrict__ prb_site,
                                                     const unsigned char* __restrict__ ref_site, int max_nodes, int exhaustive,
                                                     unsigned char* __restrict__ verdict, int32_t* __restrict__ nodes, int32_t* __restrict__ found,
                                                     int32_t* __restrict__ sites, int32_t* __restrict__ map) {
  __shared__ Pair S;
  const int64_t p = blockIdx.x;
  const int lane = threadIdx.x, idx = lane & 31, side = lane >> 5;
  const ds_rec::Pair q = ds_rec::pair_of(p, prb_rec, prb_n, ref_rec, ref_n, ref_index, M);
  ds_sites::Found r = {DSC_INVALID, -1, 0, 0, 0, 0};
  ds_sites::Census c = {0u, false, 0, 0, 0, 0};
  if (q.valid) {
    const int ng = q.n_prb(), nr = q.n_ref();
    ds_rec::load_bonds(S.adj[0], q.prb, ~0u, lane);
    ds_rec::load_bonds(S.adj[1], q.ref, ~0u, lane);
    __syncthreads();

    // the prologue per half wave: labels, neighbours, twins and ordinals of the normal form, and this node's site row
    const int mine_n = side ? nr : ng;
    const bool here = idx < mine_n;
    const unsigned char* __restrict__ rec = side ? q.ref : q.prb;
    const unsigned char* __restrict__ row = side ? ref_site + q.r * DSI_SITE_BYTES : prb_site + q.p * DSI_SITE_BYTES;
    unsigned type = 0u, fc = 0u, nbr = 0u, fl = 0u;
    int mate = 0;
    if (here) {
      type = rec[DS_REC_TYPE + idx];
      fc = rec[DS_REC_FC + idx];
      fl = row[idx * 2];
      mate = row[idx * 2 + 1];
      for (int j = 0; j < mine_n; ++j) nbr |= (S.adj[side][idx * 32 + j] ? 1u : 0u) << j;
    }
    const int deg = __popc(nbr);
    const unsigned key = ds_sites::twin_key(here ? deg : 2, __ffs((int)nbr) - 1, 0u, type, fc, lane);
    S.key[lane] = key;
    __syncthreads();
    const int ord = here ? ds_sites::count_twins(S.key + side * 32, key, mine_n, idx).ord : 0;
    // a site row that contradicts its record is no site
    const bool hslot = (fl & DSI_FLAG_HSLOT) != 0u;
    const bool centre = here && (fl & DSI_KIND_MASK) == DSI_KIND_CENTRE && deg + (hslot ? 1 : 0) == 4;
    const unsigned kept_subs = nbr & ~(1u << (mate & 31));
    const int n_subs = (int)__popc(kept_subs) + (hslot ? 1 : 0);
    const bool end = here && (fl & DSI_KIND_MASK) == DSI_KIND_END && mate < mine_n && ((nbr >> (mate & 31)) & 1u) && (n_subs == 1 || n_subs == 2);
    if (!end) mate = 0;
    const unsigned kind = centre ? DSI_KIND_CENTRE : end ? DSI_KIND_END : DSI_KIND_NONE;
    const bool assigned_here = (fl & DSI_FLAG_ASSIGNED) != 0u, sign = (fl & DSI_FLAG_SIGN) != 0u;
    const int low = end && kept_subs ? __ffs((int)kept_subs) - 1 : NO_LOW;
    const bool ez_low = end && idx < mate;                   // an E/Z site counts once, at its lower end
    c = ds_sites::census(centre, ez_low, (centre || ez_low) && !assigned_here);
    r.out = DSC_DIFFERENT;
    if (ng == nr) {
      const ds_sites::Node node = {type, fc, ord, nbr, kind, sign, hslot, mate, low};
      r = ds_sites::search(S, node, ng, lane, c.assigned, c.centres, max_nodes, exhaustive);
    }
  }
  ds_sites::write_out(p, lane, r, c, verdict, nodes, found, sites, map);
}

static_assert(DSI_MASK_MOBILE_BOND == DSC_NUM_MASKS && DSI_MASK_RING_BOND == DSC_NUM_MASKS + 1 &&
              DSI_NUM_MASKS == DSC_NUM_MASKS + 2, "flags[] in k_key_sites: the DSC_MASK_* rows (their order is asserted in ds_sites.h), then these two");
static_assert(DSI_SITE_BYTES == 2 * MA && DSI_NO_PARTNER >= MA, "a site row is (flags, partner) per node");
static_assert((DSI_KIND_MASK & (DSI_FLAG_ASSIGNED | DSI_FLAG_SIGN | DSI_FLAG_HSLOT)) == 0 && DSI_KIND_CENTRE <= DSI_KIND_MASK && DSI_KIND_END <= DSI_KIND_MASK,
              "the fields of a flags byte are apart");

}  // namespace

extern "C" int dsi_key_sites(const uint8_t* rec, const int32_t* n, int64_t P, int32_t max_nodes, double min_volume, double min_planarity,
                             uint8_t* site, int32_t* masks, double* volume, int32_t* nodes, uint8_t* status, void* stream) {
  const bool scalars_ok = max_nodes >= 1 && max_nodes <= DSM_MAX_NODES && ds_sites::thresholds_ok(min_volume, min_planarity);
  const int go = ds_rec::check_table(scalars_ok, P, rec, n, {site, masks, volume, nodes, status});
  if (go != ds_rec::LAUNCH) return go;
  hipLaunchKernelGGL(k_key_sites, dim3((unsigned)((P + DSM_WAVES - 1) / DSM_WAVES)), dim3(64 * DSM_WAVES), 0, (hipStream_t)stream, rec, n, P,
                     (int)max_nodes, min_volume, min_planarity, site, masks, volume, nodes, status);
  return DST_CHECK_LAUNCH();
}

extern "C" int dsi_key_identity_records(const uint8_t* prb_rec, const int32_t* prb_n, int64_t P, const uint8_t* ref_rec, const int32_t* ref_n,
                                        int64_t M, const int64_t* ref_index, const uint8_t* prb_site, const uint8_t* ref_site, int32_t max_nodes,
                                        int32_t exhaustive, uint8_t* verdict, int32_t* nodes, int32_t* found, int32_t* sites, int32_t* map,
                                        void* stream) {
  const bool scalars_ok = max_nodes >= 0 && max_nodes <= DS_GRAPH_MAX_NODES && (exhaustive == 0 || exhaustive == 1);
  const int go = ds_rec::check_pairs(scalars_ok, P, M, prb_rec, prb_n, ref_rec, ref_n, ref_index, {verdict, nodes, found, sites, map});
  if (go != ds_rec::LAUNCH) return go;
  if (!prb_site || (M > 0 && !ref_site)) return DS_ERR_ARG;
  hipLaunchKernelGGL(k_key_identity, dim3((unsigned)P), dim3(64), 0, (hipStream_t)stream, prb_rec, prb_n, ref_rec, ref_n, ref_index, M, prb_site,
                     ref_site, (int)max_nodes, (int)exhaustive, verdict, nodes, found, sites, map);
  return DST_CHECK_LAUNCH();
}
