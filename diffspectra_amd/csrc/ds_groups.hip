// diffspectra_amd - functional groups on result records: aromaticity perception, the 17 group predicates of the reference's "Functional Group
// Similarity" line and the two counts of their Jaccard index.  include/diffspectra_groups.h states every definition (applied charges, implicit
// hydrogens, ring bonds, the candidate / electron rule, the predicates, the unusable rule); DESIGN.md section 17 has the figures.
//
// One wave64 per record or pair, DSG_WAVES per workgroup, an atom per lane.  LDS holds, per wave, the bond matrix of ds_rec::load_bonds and
// three words per atom: its neighbours of any order, its neighbours of order 1, and its electron word (the count with the double-bond partner
// inside the cycle, the count with it outside, the partner).  A lane's ring-bond test and cycle search read other atoms' words inside divergent
// loops, so they read LDS and never shuffle; the wave-wide masks (elements, X, Ht, aromatic atoms, group bits) are ballots and one OR
// reduction outside divergent code.  Integers only, no atomics, no early exit: a wave without a record takes part in the workgroup's
// barriers and writes nothing.  From ds_perceive.h: the record scan, applied_charge and max_valence, the electron rule with ring_bond for the
// double bond, the walk over the cycles each atom is the lowest of, the wave OR.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/diffspectra_groups.h"
#include "ds_perceive.h"
#include "ds_host.h"   // DST_CHECK_LAUNCH

namespace {

using namespace ds_perceive;

struct Wave {                             // one record's staging area
  unsigned char adj[MA * 32];             // symmetric bond orders over original atom indices, diagonal 0
  unsigned any[32], one[32];              // bit j = bonded to atom j by any order / by order 1
  unsigned electrons[32];                 // bits 0-1: count with the partner in the cycle, 2-3: with it outside, 4-8: the partner
};

struct Found {                            // wave-uniform
  unsigned groups, aromatic;
  bool usable;
};

// Groups and aromatic atoms of record `mine` (not touched when n = 0: a wave without a record, or with an invalid pair, passes n = 0).  Holds
// three workgroup barriers, which every wave of the workgroup reaches: nothing in here returns early.
__device__ __forceinline__ Found analyse(Wave& S, const unsigned char* __restrict__ mine, int n, int lane) {
  const Atom A = scan(S.adj, mine, n, lane, ds_refine::Block{});
  const bool usable = usable_record(A, n), on = usable && A.active;
  const int t = min(A.type, MAX_TYPE);    // a table index whatever the byte; a type above 4 makes the record unusable
  // an unusable record has no atoms from here on: every mask is 0 and every loop below is empty
  const unsigned nb = on ? A.nb : 0u, nb1 = on ? A.nb1 : 0u, nb2 = on ? A.nb2 : 0u, nb3 = on ? A.nb3 : 0u;
  const unsigned me = lane < 32 ? 1u << lane : 0u;

  const unsigned isH = low32(__ballot(on && t == H)), isC = low32(__ballot(on && t == C)), isN = low32(__ballot(on && t == N)),
                 isO = low32(__ballot(on && t == O)), isF = low32(__ballot(on && t == F));
  const int q = applied_charge(t, A.raw);
  const int hi = max(0, max_valence(t, q) - A.val);
  const int D = __popc(nb), dbl = __popc(nb2), trp = __popc(nb3);
  const int X = D + hi, Ht = __popc(nb & isH) + hi;

  // the electron word: the counts that do not depend on the cycle now, the ring-bond test of the double bond below
  Electrons e = electron_rule(on, t, q, X, dbl, trp, nb2);
  if (lane < 32) {
    S.any[lane] = nb;
    S.one[lane] = nb1;
  }
  __syncthreads();
  if (e.partner != NO_PARTNER) e.e_out = double_bond_outside(ring_bond(S.any, me, nb, 1u << e.partner), e.partner, isN | isO);
  if (lane < 32) S.electrons[lane] = e.word();
  __syncthreads();
  const unsigned candidates = low32(__ballot(e.e_in != NONE));

  unsigned found = 0u;
  if (e.e_in != NONE)
    aromatic_cycles<true>(S.any, S.electrons, me, nb, candidates, [&](unsigned members, int, int) { found |= members; });
  const unsigned aromatic = wave_or(found);

  // the predicates: "al" = not aromatic; wave-wide masks of what a neighbour has to be, then a test per lane and a ballot per group
  const unsigned alC = isC & ~aromatic, alO = isO & ~aromatic;
  const unsigned X1 = low32(__ballot(on && X == 1)), X2 = low32(__ballot(on && X == 2)), X3 = low32(__ballot(on && X == 3));
  const unsigned Ht0 = low32(__ballot(on && Ht == 0)), Ht1 = low32(__ballot(on && Ht == 1));
  const bool al = on && !(aromatic & me);
  const bool sp2 = al && t == C && X == 3, carbonyl = (nb2 & alO) != 0u;
  const unsigned carbons = nb1 & isC;                                            // single-bonded C#
  const unsigned has_carbonyl = low32(__ballot(on && carbonyl));
  const unsigned amide_c = low32(__ballot(sp2 && (nb2 & alO & X1) && carbons));
  bool ester = false;
  if (sp2 && carbonyl && carbons)
    for (unsigned os = nb1 & alO & X2 & Ht0; os; os &= os - 1u) {                 // at most three: X = 3
      const unsigned theirs = S.one[__ffs((int)os) - 1] & isC & ~me;
      ester |= theirs && !(theirs == carbons && __popc(carbons) == 1);           // r and r' distinct: not the same single carbon on both sides
    }
  const bool is_group[15] = {
      al && t == C && X == 4,
      sp2 && (nb2 & alC & X3),
      al && t == C && X == 2 && (nb3 & alC),
      on && t == C && (aromatic & me),
      al && t == O && X == 2 && Ht == 1 && carbons,
      al && t == O && D == 2 && __popc(carbons) == 2,
      sp2 && Ht == 1 && carbonyl && carbons,
      sp2 && carbonyl && __popc(carbons) >= 2,
      sp2 && carbonyl && (nb1 & alO & X2 & Ht1),
      ester,
      on && t == F && carbons,
      sp2 && (nb2 & alO & X1) && (nb1 & isF),
      al && t == N && X == 3 && !(nb1 & alC & has_carbonyl),
      al && t == N && X == 3 && (nb1 & amide_c),
      al && t == N && X == 1 && (nb3 & alC & X2),
  };
  unsigned groups = 0u;
#pragma unroll
  for (int g = 0; g < 15; ++g) groups |= (__ballot(is_group[g]) != 0ull ? 1u : 0u) << g;
  return {usable ? groups : 0u, usable ? aromatic : 0u, usable};
}

__global__ __launch_bounds__(64 * DSG_WAVES) void k_groups(const unsigned char* __restrict__ rec, const int32_t* __restrict__ n_atoms, int64_t P,
                                                           int32_t* __restrict__ groups, int32_t* __restrict__ aromatic_mask,
                                                           unsigned char* __restrict__ status) {
  __shared__ Wave S[DSG_WAVES];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * DSG_WAVES + wave;
  const bool live = p < P;
  const int n = live ? ds_rec::atoms_of(n_atoms, p) : 0;
  const Found f = analyse(S[wave], rec + (live ? p : 0) * DS_RECORD_BYTES, n, lane);
  if (live && lane == 0) {
    groups[p] = (int32_t)f.groups;
    aromatic_mask[p] = (int32_t)f.aromatic;
    status[p] = (unsigned char)(f.usable ? DSG_OK : DSG_UNUSABLE);
  }
}

__global__ __launch_bounds__(64 * DSG_WAVES) void k_group_pairs(const unsigned char* __restrict__ prb_rec, const int32_t* __restrict__ prb_n, int64_t P,
                                                                const unsigned char* __restrict__ ref_rec, const int32_t* __restrict__ ref_n, int64_t M,
                                                                const int64_t* __restrict__ ref_index, int32_t* __restrict__ common,
                                                                int32_t* __restrict__ either, int32_t* __restrict__ groups,
                                                                unsigned char* __restrict__ status) {
  __shared__ Wave S[DSG_WAVES];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * DSG_WAVES + wave;
  const bool live = p < P;
  const ds_rec::Pair pair = ds_rec::pair_of(live ? p : 0, prb_rec, prb_n, ref_rec, ref_n, live ? ref_index : nullptr, live ? M : 0);
  const bool read = live && pair.valid;                                          // neither record nor count is touched otherwise
  const Found a = analyse(S[wave], pair.prb, read ? pair.n_prb() : 0, lane);
  const Found b = analyse(S[wave], read ? pair.ref : pair.prb, read ? pair.n_ref() : 0, lane);
  if (live && lane == 0) {
    const bool ok = read && a.usable && b.usable;
    common[p] = ok ? __popc(a.groups & b.groups) : -1;
    either[p] = ok ? __popc(a.groups | b.groups) : -1;
    groups[p * 2] = ok ? (int32_t)a.groups : 0;
    groups[p * 2 + 1] = ok ? (int32_t)b.groups : 0;
    status[p] = (unsigned char)(!read ? DSG_INVALID : ok ? DSG_OK : DSG_UNUSABLE);
  }
}

static_assert(DSG_WAVES >= 1 && 64 * DSG_WAVES <= 1024, "a workgroup of whole waves");
static_assert(DSG_NUM_GROUPS == 17, "bits 15 and 16 of the group word stay clear");

}  // namespace

extern "C" int dsg_group_records(const uint8_t* rec, const int32_t* n, int64_t P, int32_t* groups, int32_t* aromatic_mask, uint8_t* status,
                                 void* stream) {
  const int go = ds_rec::check_table(true, P, rec, n, {groups, aromatic_mask, status});
  if (go != ds_rec::LAUNCH) return go;
  hipLaunchKernelGGL(k_groups, dim3((unsigned)((P + DSG_WAVES - 1) / DSG_WAVES)), dim3(64 * DSG_WAVES), 0, (hipStream_t)stream, rec, n, P, groups,
                     aromatic_mask, status);
  return DST_CHECK_LAUNCH();
}

extern "C" int dsg_group_similarity_records(const uint8_t* prb_rec, const int32_t* prb_n, int64_t P, const uint8_t* ref_rec, const int32_t* ref_n,
                                            int64_t M, const int64_t* ref_index, int32_t* common, int32_t* either, int32_t* groups,
                                            uint8_t* status, void* stream) {
  const int go = ds_rec::check_pairs(true, P, M, prb_rec, prb_n, ref_rec, ref_n, ref_index, {common, either, groups, status});
  if (go != ds_rec::LAUNCH) return go;
  hipLaunchKernelGGL(k_group_pairs, dim3((unsigned)((P + DSG_WAVES - 1) / DSG_WAVES)), dim3(64 * DSG_WAVES), 0, (hipStream_t)stream, prb_rec, prb_n, P,
                     ref_rec, ref_n, M, ref_index, common, either, groups, status);
  return DST_CHECK_LAUNCH();
}
