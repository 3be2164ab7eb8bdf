// diffspectra_amd - what the stereo level (ds_stereo.hip: records as drawn) and the key level (ds_key.hip: normal forms with site rows) share:
// twins and ordinals, the fp64 geometry of a site, and the pair search that goes on after a verified leaf and tests every isomorphism against
// the site bits in integers.  The key level is the general form - a site may stand on a hydrogen slot, and the sites come from rows that the
// search cannot trust to be respected by an isomorphism - and the stereo level is the case without a slot.  The definitions are those of
// include/diffspectra_stereo.h and include/diffspectra_key.h; DESIGN.md sections 21 and 25.
//
// The pieces of the search (verify, open_level, next_try, individualise) are ds_refine.h's.  k_graph_identity (ds_graph.hip) and k_smiles
// (ds_smiles.hip) keep their own loops over them: the first stops at its first leaf and has no sites, the second is a one-molecule walk.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/diffspectra_key.h"   // the DSI_KIND_* / DSI_FLAG_* bits of a staged site byte; it includes diffspectra_stereo.h
#include "ds_records.h"
#include "ds_refine.h"
#include "ds_vec.h"

namespace ds_sites {

using ds_rec::MA;
using namespace ds_vec;

constexpr unsigned HSLOT = 1u << 31;      // in a substituent word: the end has a hydrogen slot (atoms are bits 0..28)
constexpr int NO_LOW = 31;                // "lowest substituent" of a node that is no end, or of an end whose only substituent is its hydrogen slot
static_assert(MA <= 29, "bits 29..31 of an atom mask are free: HSLOT, NO_LOW");
static_assert(DSC_MASK_TETRA_SITE == 0 && DSC_MASK_TETRA_ASSIGNED == 1 && DSC_MASK_TETRA_POSITIVE == 2 && DSC_MASK_EZ_SITE == 3 &&
              DSC_MASK_EZ_ASSIGNED == 4 && DSC_MASK_EZ_CIS == 5 && DSC_MASK_TWIN == 6, "the order of the mask rows in k_stereo_sites and k_key_sites");

__device__ __forceinline__ unsigned half_of(unsigned long long ballot, int side) { return (unsigned)(ballot >> (32 * side)); }
inline bool thresholds_ok(double min_volume, double min_planarity) { return min_volume >= 0.0 && min_planarity >= 0.0; }   // false for a NaN

// ------------------------------------------------------------------------------------------------------------------ twins and ordinals
// Twin key: a leaf's is (parent, order, type, charge byte), a bondless atom's (type, charge byte), every other atom's is its own.  The stereo
// level passes the order of the leaf's bond: on a record as drawn =O and -O on one atom are different substituents.  The key level passes 0:
// every bond of a normal form is byte 1, and the orders of the original are what mobile hydrogens and Kekule drawings move about.
__device__ __forceinline__ unsigned twin_key(int degree, int parent, unsigned order, unsigned type, unsigned charge, int self) {
  return degree == 1 ? 1u << 29 | (unsigned)parent << 24 | order << 16 | type << 8 | charge
                     : degree == 0 ? 2u << 29 | type << 8 | charge : 3u << 29 | (unsigned)self;
}

struct Twins { int ord; bool twin; };     // atoms below this one with its key; whether any other atom has it

__device__ __forceinline__ Twins count_twins(const unsigned* keys, unsigned key, int n, int idx) {
  Twins t = {0, false};
  for (int j = 0; j < n; ++j) {
    const bool same = keys[j] == key;
    t.ord += same && j < idx;
    t.twin |= same && j != idx;
  }
  return t;
}

// ------------------------------------------------------------------------------------------------------------------ the geometry of a site
// at(atom) -> ds_vec::Vec is the caller's position lookup: fp32 record values widened to fp64.

// Signed volume over the unit vectors from `self` to its four neighbours: those of `nbr` in ascending index, then `last` (the hydrogen behind
// the slot) when `nbr` holds three.  fin = every position read is finite.
template <class At>
__device__ __forceinline__ double tetra_volume(At at, int self, unsigned nbr, int last, bool& fin) {
  const Vec x = at(self);
  fin = finite(x);
  unsigned m = nbr;
  auto unit = [&]() {
    const int j = m ? __ffs((int)m) - 1 : last;
    m &= m - 1u;
    const Vec y = at(j);
    fin &= finite(y);
    const Vec d = y - x;
    return d * (1.0 / sqrt(dot(d, d)));
  };
  const Vec u1 = unit(), u2 = unit(), u3 = unit(), u4 = unit();
  return dot(u1 - u4, cross(u2 - u4, u3 - u4));
}

// The E/Z site of the double bond a = b, worked out by its lower end: bit 0 = assigned (every position finite, every |cosine| of the one to
// four substituent pairs at least min_planarity, and the pairs consistent: two substituents of one end lie on opposite sides), bit 1 = cis (of
// the lowest substituents).  subs / mate_subs: the substituent atoms of a / b as bits, HSLOT = and the hydrogen h_a / h_b, which counts last.
template <class At>
__device__ __forceinline__ unsigned ez_result(At at, int a, int b, unsigned subs, unsigned mate_subs, int h_a, int h_b, double min_planarity) {
  const Vec xa = at(a), xb = at(b), e = xb - xa;
  const double ee = dot(e, e);
  bool ok = finite(xa) && finite(xb);
  unsigned cis = 0u;
  int k = 0;                               // pair (i-th substituent of a, j-th of b) -> bit i * nt + j
  const auto atom_of = [](unsigned word, int h) { return (word & ~HSLOT) ? __ffs((int)(word & ~HSLOT)) - 1 : h; };
  const auto rest_of = [](unsigned word) { return (word & ~HSLOT) ? word & (word - 1u) : 0u; };
  for (unsigned sm = subs; sm; sm = rest_of(sm))
    for (unsigned tm = mate_subs; tm; tm = rest_of(tm), ++k) {
      const Vec xs = at(atom_of(sm, h_a)), xt = at(atom_of(tm, h_b));
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
  return (ok ? 1u : 0u) | (cis & 1u) << 1;
}

// ------------------------------------------------------------------------------------------------------------------ the pair search
// One wave64 per pair, one wave per workgroup: the generated molecule in lanes 0..28, the ground truth in lanes 32..60, as k_graph_identity.

struct Node {                             // what a lane knows of its atom when the search starts
  unsigned type, fc;                      // type byte, charge byte
  int ord;                                // twin ordinal
  unsigned nbr;                           // bit j = bonded to atom j of the own side
  unsigned kind;                          // DSI_KIND_NONE / _CENTRE / _END
  bool sign, hslot;                       // V > 0 of a centre, the cis bit of an end; the site has a hydrogen slot
  int mate, low;                          // of an end: the other end, the lowest substituent that is an atom (NO_LOW: none); 0 and NO_LOW off-site
};

struct Census { unsigned centres; bool assigned; int tetra_a, ez_a, open_a, open_b; };
struct Found { int out, image, used, isos, sames, mirrors; };

// The sites of both molecules counted: centre / ez_low (the lower end of an E/Z site: a site counts once) / open (a site that is not assigned)
// of this lane.  centres = the generated molecule's; assigned = no site of either molecule is open.
__device__ __forceinline__ Census census(bool centre, bool ez_low, bool open_here) {
  const unsigned centres = half_of(__ballot(centre), 0);
  const unsigned long long open = __ballot(open_here);
  return {centres, open == 0ull, (int)__popc(centres), (int)__popc(half_of(__ballot(ez_low), 0)), (int)__popc(half_of(open, 0)), (int)__popc(half_of(open, 1))};
}

// The search of two molecules of n atoms each.  The Store is that of ds_refine.h's pair search plus `unsigned char type[64], fc[64], ord[64],
// flag[64], mate[64], low[64]`, which are staged here.  The initial colour and verify()'s labels hold (type, charge, ordinal), and the search
// goes on after a verified leaf, so that it meets every ordinal-respecting isomorphism exactly once (the argument stands in ds_refine.h).
//
// Soundness, in the lines the code keeps true: a leaf counts only after ds_refine::verify() has compared every type, charge, ordinal and bond
// byte under an explicit bijection; DSC_DIFFERENT needs an exhausted search without such a leaf; DSC_MIRROR / DSC_STEREOISOMER need an
// exhausted search, so that no same phi was missed; a search the budget stops is DSC_UNDECIDED whatever it had found.
//
// The leaf test, when every site of both molecules is assigned: an isomorphism has to send sites onto sites (`off`: the same kind and slot flag
// at the image, which is a bijection, so the ground truth's sites are then all met; the partner's image is the image's partner - true of
// every isomorphism at the stereo level, where twins, degrees and orders make the sites, and checked all the same).  A centre keeps its sign
// times the parity of the order of its neighbours' images; a hydrogen slot goes to the hydrogen slot, last on both sides (d = 64).  An E/Z
// site keeps its cis bit, flipped once per end whose lowest substituent goes elsewhere than to the lowest substituent of the image.
// Found.image = this lane's image (-1: not a generated atom, or the verdict has no map) under the first isomorphism of the verdict's kind.
template <class Store>
__device__ __forceinline__ Found search(Store& S, const Node& node, int n, int lane, bool assigned, unsigned centres, int max_nodes, int exhaustive) {
  const int idx = lane & 31, side = lane >> 5;
  const bool active = idx < n, centre = node.kind == DSI_KIND_CENTRE, end = node.kind == DSI_KIND_END;
  S.type[lane] = (unsigned char)node.type;
  S.fc[lane] = (unsigned char)node.fc;
  S.ord[lane] = (unsigned char)node.ord;
  S.flag[lane] = (unsigned char)(node.kind | (node.sign ? DSI_FLAG_SIGN : 0u) | (node.hslot && node.kind ? DSI_FLAG_HSLOT : 0u));
  S.mate[lane] = (unsigned char)node.mate;
  S.low[lane] = (unsigned char)node.low;
  __syncthreads();
  // initial colour: (type, charge, ordinal) ranked jointly
  const ds_refine::Ranked first = ds_refine::rank_jointly<true>(S, (unsigned long long)(node.type << 16 | node.fc << 8 | (unsigned)node.ord), n, lane, ds_refine::Block{});
  int colour = active ? first.colour : 0;
  unsigned long long multi = 0ull;
  int st = __ballot(active && first.eq_g != first.eq_r) ? ds_refine::MISMATCH : ds_refine::refine<true>(S, colour, active, n, lane, multi, ds_refine::Block{});
  int depth = 0;                                             // open levels: S.stack[0 .. depth-1]
  int used = 0, isos = 0, sames = 0, mirrors = 0;            // (plain ints, made a Found at the return: as members they go to scratch)
  int first_iso = -1, first_same = -1, first_mirror = -1;    // this lane's image under the first isomorphism of each kind
  bool ended = false;                                        // the search stopped for another reason than the budget
  const auto same_label = [&S](int a, int b) { return S.type[a] == S.type[b] && S.fc[a] == S.fc[b] && S.ord[a] == S.ord[b]; };
  for (int it = 0; it <= max_nodes; ++it) {                  // every pass but the last spends one search node
    if (st == ds_refine::DISCRETE && ds_refine::verify(S, colour, active, n, lane, same_label)) {
      const int to = active && side == 0 ? S.img[idx] : -1;
      if (isos++ == 0) first_iso = to;
      bool same = false;
      if (assigned) {
        bool off = false, inverted = false, ez_bad = false;
        if (side == 0 && active) {
          const unsigned there = S.flag[32 + to];
          off = ((there ^ S.flag[lane]) & (DSI_KIND_MASK | DSI_FLAG_HSLOT)) != 0u || (end && S.img[node.mate] != S.mate[32 + to]);
          if (centre && !off) {
            unsigned m = node.nbr;
            const int a = S.img[__ffs((int)m) - 1]; m &= m - 1u;
            const int b = S.img[__ffs((int)m) - 1]; m &= m - 1u;
            const int c = S.img[__ffs((int)m) - 1]; m &= m - 1u;
            const int d = m ? S.img[__ffs((int)m) - 1] : 64;
            const unsigned odd = (unsigned)((a > b) + (a > c) + (a > d) + (b > c) + (b > d) + (c > d)) & 1u;
            inverted = (node.sign ? 1u : 0u) != ((there & DSI_FLAG_SIGN ? 1u : 0u) ^ odd);
          }
          if (end && !off) {
            const int mate_to = S.img[node.mate], mate_low = S.low[node.mate];
            const unsigned flips = (node.low != NO_LOW && S.img[node.low] != S.low[32 + to] ? 1u : 0u) ^
                                   (mate_low != NO_LOW && S.img[mate_low & 31] != S.low[32 + mate_to] ? 1u : 0u);
            ez_bad = (node.sign ? 1u : 0u) != ((there & DSI_FLAG_SIGN ? 1u : 0u) ^ flips);
          }
        }
        const bool onto = __ballot(off) == 0ull;
        const unsigned turned = half_of(__ballot(inverted), 0);
        const bool ez_kept = __ballot(ez_bad) == 0ull;
        same = onto && turned == 0u && ez_kept;
        if (same && sames++ == 0) first_same = to;
        if (onto && centres != 0u && turned == centres && ez_kept && mirrors++ == 0) first_mirror = to;
      }
      if (!exhaustive && (same || !assigned)) { ended = true; break; }
    }
    if (st == ds_refine::CELLS) {
      if (depth >= MA) break;                                // (cannot happen: every level makes one more generated atom a class of its own)
      ds_refine::open_level(S, depth, colour, active, lane, multi);
    }
    const ds_refine::Try t = ds_refine::next_try(S, depth, colour, active, lane);
    if (t.w < 0) { ended = true; break; }                    // nothing left to try anywhere: every isomorphism has been met
    if (used >= max_nodes) break;                            // the budget does not cover this try: undecided
    ++used;
    st = ds_refine::individualise(S, depth, t, colour, active, n, lane, multi);
  }
  int out = DSC_UNDECIDED, image = -1;
  if (ended) {
    if (isos == 0) out = DSC_DIFFERENT;
    else if (!assigned) { out = DSC_UNASSIGNED; image = first_iso; }
    else if (sames) { out = DSC_IDENTICAL; image = first_same; }
    else if (mirrors) { out = DSC_MIRROR; image = first_mirror; }
    else { out = DSC_STEREOISOMER; image = first_iso; }
  }
  return {out, image, used, isos, sames, mirrors};
}

// what both identity kernels write of pair p (the structs by value: behind references their members are kept in scratch)
__device__ __forceinline__ void write_out(int64_t p, int lane, Found r, Census c, unsigned char* __restrict__ verdict,
                                          int32_t* __restrict__ nodes, int32_t* __restrict__ found, int32_t* __restrict__ sites, int32_t* __restrict__ map) {
  if (lane < MA) map[p * MA + lane] = r.image;
  if (lane < 3) found[p * 3 + lane] = lane == 0 ? r.isos : lane == 1 ? r.sames : r.mirrors;
  if (lane < 4) sites[p * 4 + lane] = lane == 0 ? c.tetra_a : lane == 1 ? c.ez_a : lane == 2 ? c.open_a : c.open_b;
  if (lane == 0) {
    verdict[p] = (unsigned char)r.out;
    nodes[p] = r.used;
  }
}

}  // namespace ds_sites
