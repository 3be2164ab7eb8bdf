// diffspectra_amd - BRICS analytics on result records: the environments of every atom, the retrosynthetic cuts with their labels, the fragment
// of every atom, and the fragments as records of their own, behind the "Frag" number of the reference's set metrics.
// include/diffspectra_brics.h states every definition (the matchable graph, the thirteen environments, the forty rules and their order, the
// both-orientations rule, fragments and attachment points, the unusable rule); DESIGN.md section 22 has the method and the figures.
//
// One wave64 per record, DSB_WAVES records per workgroup, an atom per lane.  `analyse` starts from ds_perceive::matched_graph, the perception
// that the prologue of ds_substructure.hip runs too (the record scan, the fold, ring_bond for every bond, the electron rule, the cycle walk
// through the lane's OWN atom, which gives it its aromatic-bond neighbours without a scatter); it keeps the lane's bond-class masks in
// registers, because an environment reads the classes of its own atom only - what it needs of the neighbours (element, aromaticity, "a C
// with a double bond to O") are ballots.  LDS holds, per wave, the bond matrix, the neighbour masks of the
// perception, the environment word of every atom for the rule walk of the lower bond end, the cuts that walk found, the label of either end
// of a cut, the matchable neighbours without the cuts, and the lowest atom every atom reaches over them.  The fragment kernel composes a row
// in LDS and stores it as dwords; its loop over the fragments of a record runs a different number of times in every wave, so it holds wave
// barriers only.  Integers only, no atomics, no early exit: a wave without a record takes part in the workgroup's barriers and writes nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/diffspectra_brics.h"
#include "ds_perceive.h"
#include "ds_host.h"   // DST_CHECK_LAUNCH

namespace {

using namespace ds_perceive;

// The rules of the header in their order: bits 0-4 x, bits 5-9 y, bit 10 = a double bond.
#define DSB_RULE(x, y) ((x) | ((y) << 5))
static __constant__ unsigned short c_rules[DSB_NUM_RULES] = {
    DSB_RULE(1, 3),   DSB_RULE(1, 5),   DSB_RULE(1, 10),
    DSB_RULE(3, 4),   DSB_RULE(3, 13),  DSB_RULE(3, 14),  DSB_RULE(3, 15),  DSB_RULE(3, 16),
    DSB_RULE(4, 5),
    DSB_RULE(5, 14),  DSB_RULE(5, 16),  DSB_RULE(5, 13),  DSB_RULE(5, 15),
    DSB_RULE(6, 13),  DSB_RULE(6, 14),  DSB_RULE(6, 15),  DSB_RULE(6, 16),
    DSB_RULE(7, 7) | (1 << 10),
    DSB_RULE(8, 9),   DSB_RULE(8, 10),  DSB_RULE(8, 13),  DSB_RULE(8, 14),  DSB_RULE(8, 15),  DSB_RULE(8, 16),
    DSB_RULE(9, 13),  DSB_RULE(9, 14),  DSB_RULE(9, 15),  DSB_RULE(9, 16),
    DSB_RULE(10, 13), DSB_RULE(10, 14), DSB_RULE(10, 15), DSB_RULE(10, 16),
    DSB_RULE(13, 14), DSB_RULE(13, 15), DSB_RULE(13, 16),
    DSB_RULE(14, 14), DSB_RULE(14, 15), DSB_RULE(14, 16),
    DSB_RULE(15, 16),
    DSB_RULE(16, 16)};
#undef DSB_RULE

struct Wave {                             // one record's staging area
  unsigned char adj[MA * 32];             // symmetric bond orders over original atom indices, diagonal 0
  unsigned char label[MA * 32];           // [a * 32 + b]: the label of atom a on the cut a-b; written and read for cuts only
  unsigned any[32];                       // bit j = bonded to atom j by any order
  unsigned matched[32];                   // the same among matchable atoms, 0 for a folded hydrogen
  unsigned electrons[32];                 // the electron word of ds_perceive::Electrons
  unsigned env[32];                       // bit e = the atom is in L_e
  unsigned cut_up[32];                    // bit b = the bond to atom b > this atom is a cut (the lower end walks the rules)
  unsigned kept[32];                      // the matchable neighbours without the cuts
  unsigned lowest[32];                    // the lowest atom reached over `kept`
};

struct Found {                            // what the analysis leaves; matchable, roots, cuts and fragments are wave-uniform
  bool usable, on, node;                  // the record is usable / and this lane holds an atom / and that atom is matchable
  int charge;                             // the applied charge of this lane's atom
  unsigned nb, aromatic_nb, cut_nb;       // bonded by any order / by an aromatic bond / by a cut
  unsigned env, cut_up;
  unsigned matchable, roots;              // roots: the lowest atom of every fragment
  int fragment;                           // of this lane's atom, -1 for a lane without one
  int cuts, fragments;
};

// Holds seven workgroup barriers, which every wave of the workgroup reaches.  n = 0: a wave without a record; `mine` is not touched.
__device__ __forceinline__ Found analyse(Wave& S, const unsigned char* __restrict__ mine, int n, int lane) {
  const Matched M = matched_graph(S.adj, S.any, S.matched, S.electrons, mine, n, lane, [](unsigned) {});
  const bool usable = M.usable, on = M.on, node = M.node;
  const int t = M.t, q = M.q;
  const unsigned nb = M.nb, nb1 = M.nb1, nb2 = M.nb2, matchable = M.matchable, ring_nb = M.ring_nb, arom_nb = M.arom_nb;
  const unsigned isH = M.isH, isN = M.isN, isO = M.isO, isC = low32(__ballot(on && t == C)), isF = low32(__ballot(on && t == F));
  const unsigned me = lane < 32 ? 1u << lane : 0u;
  const unsigned mnb = node ? nb & matchable : 0u;
  const unsigned aromatic = low32(__ballot(arom_nb != 0u));

  // the bond classes of this atom: single / double by chain / ring, aromatic; all among matchable atoms
  const unsigned plain = mnb & ~arom_nb, ar = mnb & arom_nb;
  const unsigned single = nb1 & plain, dbl = nb2 & plain;
  const unsigned s_chain = single & ~ring_nb, s_ring = single & ring_nb, d_chain = dbl & ~ring_nb;
  const unsigned ring_m = mnb & ring_nb;                                          // a ring bond of any kind
  const bool arom = arom_nb != 0u, in_ring = ring_nb != 0u;
  const int D = __popc(mnb);

  // the environments: upper case = not aromatic, lower case = aromatic
  const unsigned Cu = isC & ~aromatic, Nu = isN & ~aromatic, Ou = isO & ~aromatic, cno = isC | isN | isO, CNOu = Cu | Nu | Ou;
  const bool aC = node && t == C && !arom, aN = node && t == N && !arom, aO = node && t == O && !arom;
  const unsigned carbonyl = low32(__ballot(aC && (dbl & Ou)));                    // a C with a double bond to O
  const bool lactam = aN && (ring_m & carbonyl);
  unsigned env = 0u;
  if (aC && D == 3 && (dbl & Ou) && __popc(mnb & cno) >= 2) env |= 1u << 1;
  if (aO && D == 2 && (s_chain & (isC | isH))) env |= 1u << 3;
  if (aC && D != 1 && !dbl && (s_chain & isC)) env |= 1u << 4;
  if (aN && D != 1 && !dbl && !(single & (isN | isO | isF)) && !lactam) env |= 1u << 5;
  if (aC && !in_ring && D == 3 && (dbl & Ou) && (s_chain & cno)) env |= 1u << 6;
  if (aC && (D == 2 || D == 3) && (single & isC)) env |= 1u << 7;
  if (aC && !in_ring && D != 1 && mnb == single) env |= 1u << 8;
  if (node && t == N && arom && q == 0 && __popc(ar & cno) >= 2) env |= 1u << 9;
  if (aN && (ring_m & carbonyl) && __popc(ring_m & CNOu) >= 2) env |= 1u << 10;
  if (aC && (s_ring & (Nu | Ou)) && __popc(s_ring & CNOu) >= 2) env |= 1u << 13;
  if (node && t == C && arom && (ar & (isN | isO)) && __popc(ar & cno) >= 2) env |= 1u << 14;
  if (aC && __popc(s_ring & Cu) >= 2) env |= 1u << 15;
  if (node && t == C && arom && __popc(ar & isC) >= 2) env |= 1u << 16;
  if (lane < 32) S.env[lane] = env;
  __syncthreads();

  // the cuts: the lower end of every chain single or double bond walks the rules; the first that fits in either orientation decides
  const unsigned above = lane < 32 ? ~((me << 1) - 1u) : 0u;
  unsigned cut_up = 0u;
  for (unsigned left = (s_chain | d_chain) & above; left; left &= left - 1u) {
    const int b = __ffs((int)left) - 1;
    const unsigned other = S.env[b], is_double = (d_chain >> b) & 1u;
    for (int r = 0; r < DSB_NUM_RULES; ++r) {
      const unsigned w = c_rules[r], x = w & 31u, y = (w >> 5) & 31u;
      if ((w >> 10) != is_double) continue;
      const unsigned fwd = (env >> x) & (other >> y) & 1u, rev = (env >> y) & (other >> x) & 1u;
      if (fwd | rev) {
        cut_up |= 1u << b;
        S.label[lane * 32 + b] = (unsigned char)(fwd ? x : y);
        S.label[b * 32 + lane] = (unsigned char)(rev ? x : y);
        break;
      }
    }
  }
  if (lane < 32) S.cut_up[lane] = cut_up;
  __syncthreads();
  unsigned cut_nb = cut_up;                                                       // and the cuts the lower ends found to this atom
  for (unsigned left = (s_chain | d_chain) & ~above & ~me; left; left &= left - 1u) {
    const int a = __ffs((int)left) - 1;
    if ((S.cut_up[a] >> lane) & 1u) cut_nb |= 1u << a;
  }
  if (lane < 32) S.kept[lane] = mnb & ~cut_nb;
  __syncthreads();

  // fragments: the lowest atom a matchable atom reaches without the cuts; a folded hydrogen goes with its neighbour
  unsigned low = 0u;
  if (node) {
    const unsigned reached = reach(S.kept, me, me, 0u);
    low = (unsigned)(__ffs((int)reached) - 1);
  }
  if (lane < 32) S.lowest[lane] = low;
  __syncthreads();
  if (on && !node) low = S.lowest[__ffs((int)nb) - 1];
  const unsigned roots = low32(__ballot(node && low == (unsigned)lane));
  const int fragment = on ? (int)__popc(roots & ((1u << low) - 1u)) : -1;
  return {usable, on, node, q, nb, ar, cut_nb, env, cut_up, matchable, roots, fragment, wave_sum((int)__popc(cut_up)), (int)__popc(roots)};
}

__global__ __launch_bounds__(64 * DSB_WAVES) void k_brics(const unsigned char* __restrict__ rec, const int32_t* __restrict__ n_atoms, int64_t P,
                                                          int32_t* __restrict__ env, unsigned char* __restrict__ cuts,
                                                          unsigned char* __restrict__ fragment_of, int32_t* __restrict__ summary,
                                                          unsigned char* __restrict__ status) {
  __shared__ Wave W[DSB_WAVES];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * DSB_WAVES + wave;
  const bool live = p < P;
  const int n = live ? ds_rec::atoms_of(n_atoms, p) : 0;            // a wave without a record passes n = 0 and touches no record
  Wave& S = W[wave];
  const Found r = analyse(S, rec + (live ? p : 0) * DS_RECORD_BYTES, n, lane);

  // where this lane's cuts go: behind those of the lanes below it
  const int mine = (int)__popc(r.cut_up);
  int row = 0;
  for (int j = 0; j < n; ++j) {
    const int c = __shfl(mine, j, 64);
    if (j < lane) row += c;
  }
  // the largest fragment, hydrogens included
  int largest = 0;
  for (int f = 0; f < r.fragments; ++f) largest = max(largest, (int)__popcll(__ballot(r.on && r.fragment == f)));

  if (live) {
    if (lane < MA) {
      env[p * MA + lane] = (int32_t)r.env;                                        // 0 for a folded hydrogen, for atoms >= n, for an unusable record
      fragment_of[p * MA + lane] = (unsigned char)(r.on ? r.fragment : 0xff);
    }
    unsigned char* __restrict__ out = cuts + p * (DSB_MAX_CUTS * 4);
    for (unsigned left = r.cut_up; left && row < DSB_MAX_CUTS; left &= left - 1u, ++row) {
      const int b = __ffs((int)left) - 1;
      out[row * 4 + 0] = (unsigned char)lane;
      out[row * 4 + 1] = (unsigned char)b;
      out[row * 4 + 2] = S.label[lane * 32 + b];
      out[row * 4 + 3] = S.label[b * 32 + lane];
    }
    if (lane < DSB_MAX_CUTS && lane >= r.cuts)
      for (int k = 0; k < 4; ++k) out[lane * 4 + k] = 0xff;
    if (lane < 4) {
      const int v = lane == 0 ? __popc(r.matchable) : lane == 1 ? r.cuts : lane == 2 ? r.fragments : largest;
      summary[p * 4 + lane] = r.usable ? v : 0;
    }
    if (lane == 0) status[p] = (unsigned char)(r.usable ? DSB_OK : DSB_UNUSABLE);
  }
}

struct Row {                              // the fragment kernel's staging area: the analysis and one output row
  Wave w;
  alignas(16) unsigned char out[DS_RECORD_BYTES];
};

__global__ __launch_bounds__(64 * DSB_WAVES) void k_brics_fragments(const unsigned char* __restrict__ rec, const int32_t* __restrict__ n_atoms, int64_t P,
                                                                    const int64_t* __restrict__ first, int64_t F, int aromatic,
                                                                    unsigned char* __restrict__ out_rec, int32_t* __restrict__ out_n,
                                                                    int64_t* __restrict__ out_owner, unsigned char* __restrict__ out_source) {
  __shared__ Row W[DSB_WAVES];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * DSB_WAVES + wave;
  const bool live = p < P;
  const int n = live ? ds_rec::atoms_of(n_atoms, p) : 0;
  Wave& S = W[wave].w;
  unsigned char* row = W[wave].out;                                               // bytes and dwords of one array: no __restrict__
  uint32_t* row_words = reinterpret_cast<uint32_t*>(row);
  const unsigned char* __restrict__ mine = rec + (live ? p : 0) * DS_RECORD_BYTES;
  const Found r = analyse(S, mine, n, lane);
  const int64_t base = live ? first[p] : 0;
  const unsigned me = lane < 32 ? 1u << lane : 0u;
  const ds_refine::Wave sync{};                                                    // every wave runs its own number of rounds: no workgroup barrier below

  for (int f = 0; f < r.fragments; ++f) {                                         // wave-uniform; an unusable record has no fragment
    const int64_t at = base + f;
    if (at < 0 || at >= F) continue;
    const unsigned members = low32(__ballot(r.on && r.fragment == f));
    const unsigned attached = low32(__ballot(r.node && !(members & me) && (r.cut_nb & members)));      // the outside atoms, one cut each
    const int m = (int)__popc(members), total = m + (int)__popc(attached);
    for (int w = lane; w < DS_RECORD_BYTES / 4; w += 64) row_words[w] = 0u;
    sync();
    const bool member = (members & me) != 0u, outside = (attached & me) != 0u;
    const int slot = member ? (int)__popc(members & (me - 1u)) : outside ? m + (int)__popc(attached & (me - 1u)) : MA;
    if (slot < MA) {                                                              // (members + attachment points <= n: the header's argument)
      const uint32_t* __restrict__ words = reinterpret_cast<const uint32_t*>(mine);
      for (int k = 0; k < 3; ++k) row_words[DS_REC_POS / 4 + slot * 3 + k] = words[DS_REC_POS / 4 + lane * 3 + k];
      if (member) {
        row[DS_REC_TYPE + slot] = mine[DS_REC_TYPE + lane];
        row[DS_REC_FC + slot] = (unsigned char)(signed char)r.charge;
        for (unsigned left = r.nb & members; left; left &= left - 1u) {
          const int j = __ffs((int)left) - 1;
          const bool ring = aromatic && ((r.aromatic_nb >> j) & 1u);
          row[DS_REC_BOND + slot * MA + (int)__popc(members & ((1u << j) - 1u))] = ring ? (unsigned char)DSB_AROMATIC_ORDER : S.adj[lane * 32 + j];
        }
      } else {
        const int inside = __ffs((int)(r.cut_nb & members)) - 1, to = (int)__popc(members & ((1u << inside) - 1u));
        row[DS_REC_TYPE + slot] = (unsigned char)DSB_ATTACH_TYPE;
        row[DS_REC_FC + slot] = S.label[inside * 32 + lane];
        row[DS_REC_BOND + slot * MA + to] = row[DS_REC_BOND + to * MA + slot] = S.adj[lane * 32 + inside];
      }
      out_source[at * MA + slot] = (unsigned char)lane;
    }
    if (lane < MA && lane >= total) out_source[at * MA + lane] = 0xff;
    if (lane == 0) {
      out_n[at] = total;
      out_owner[at] = p;
    }
    sync();
    uint32_t* __restrict__ dst = reinterpret_cast<uint32_t*>(out_rec + at * DS_RECORD_BYTES);
    for (int w = lane; w < DS_RECORD_BYTES / 4; w += 64) dst[w] = row_words[w];
    sync();                                                                       // the next round clears the row
  }
}

static_assert(DSB_WAVES >= 1 && 64 * DSB_WAVES <= 1024, "a workgroup of whole waves");
static_assert(DSB_MAX_CUTS == MA - 1 && DS_REC_POS % 4 == 0 && DS_RECORD_BYTES % 4 == 0, "bridges of a graph on MA atoms; positions and rows as dwords");
static_assert(DSB_ATTACH_TYPE > MAX_TYPE && DSB_AROMATIC_ORDER > MAX_ORDER, "fragment records are outside the alphabet of the analytics");

}  // namespace

extern "C" int dsb_brics_records(const uint8_t* rec, const int32_t* n, int64_t P, int32_t* env, uint8_t* cuts, uint8_t* fragment_of, int32_t* summary,
                                 uint8_t* status, void* stream) {
  const int go = ds_rec::check_table(true, P, rec, n, {env, cuts, fragment_of, summary, status});
  if (go != ds_rec::LAUNCH) return go;
  hipLaunchKernelGGL(k_brics, dim3((unsigned)((P + DSB_WAVES - 1) / DSB_WAVES)), dim3(64 * DSB_WAVES), 0, (hipStream_t)stream, rec, n, P, env, cuts,
                     fragment_of, summary, status);
  return DST_CHECK_LAUNCH();
}

extern "C" int dsb_brics_fragment_records(const uint8_t* rec, const int32_t* n, int64_t P, const int64_t* first, int64_t F, int32_t aromatic,
                                          uint8_t* out_rec, int32_t* out_n, int64_t* out_owner, uint8_t* out_source, void* stream) {
  const int go = ds_rec::check_table((aromatic == 0 || aromatic == 1) && F >= 0, P, rec, n, {first, out_rec, out_n, out_owner, out_source});
  if (go != ds_rec::LAUNCH) return go;
  if (reinterpret_cast<uintptr_t>(out_rec) & 3) return DS_ERR_ARG;                // rows are stored as dwords
  hipLaunchKernelGGL(k_brics_fragments, dim3((unsigned)((P + DSB_WAVES - 1) / DSB_WAVES)), dim3(64 * DSB_WAVES), 0, (hipStream_t)stream, rec, n, P,
                     first, F, (int)aromatic, out_rec, out_n, out_owner, out_source);
  return DST_CHECK_LAUNCH();
}
