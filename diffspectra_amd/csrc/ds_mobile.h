// diffspectra_amd - the mobile-hydrogen analysis of one result record by one wave64, an atom per lane: what ds_mobile.hip (the groups and the
// normal form) and ds_key.hip (the stereo sites at the normalised level) share.  include/diffspectra_mobile.h states every definition (the
// fold, the charge normalisation, donors, acceptors and interior atoms, the simple alternating shift path, the groups, the search order and
// its budget); DESIGN.md section 23 has the method.
//
// The scan, the fold, the applied charge and Vmax are those of ds_perceive.h.  An interior atom has one double bond, so a shift path is a
// chain of extensions (over a single bond to an interior atom, on over that atom's double bond); every donor lane runs the depth-first search
// over them on its own, with its stack - the extensions still to try at every level, and the two atoms a level put on the path - in LDS,
// because a stack in registers indexed by the depth would go to scratch.  The lanes of a wave diverge inside that loop only; every wave works
// on its own LDS area, so the callers hold wave barriers only and a wave without a record runs through with n = 0.  Integers only, no atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/diffspectra_mobile.h"
#include "ds_perceive.h"

namespace ds_mobile {

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
  // what ds_key.hip reads on (a caller that does not costs it nothing): all 0 in an unusable record
  bool donor, moved;                      // this lane's atom is a donor / gave or took a proton under rule 2
  int type;                               // its type as a table index
  unsigned nb, nb2, nb3, folded;          // its neighbours by any order / by order 2 / 3; the folded hydrogens of the record (wave-uniform)
  unsigned acceptors, interior;           // wave-uniform
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
  return {status, kept_atom, member, q_res, ht, group, nb & kept, kept, comp, roots, (int)__popc(roots), p, nodes, mobile,
          donor, dp != 0, t, nb, nb2, nb3, folded, acceptors, interior};
}

// the mobile H of the group whose lowest atom is this lane's (asked by the root lanes only)
__device__ __forceinline__ int group_hydrogens(const Wave& S, unsigned comp) {
  int h = 0;
  for (unsigned m = comp; m; m &= m - 1u) h += S.ht[__ffs((int)m) - 1];
  return h;
}

static_assert(DSM_MAX_GROUPS == MA / 2 && DSM_LEVELS >= (MA - 1) / 2 + 1, "groups of two atoms at least; a simple path of MA atoms has (MA - 1) / 2 extensions");
static_assert(DSM_MAX_NODES <= (0x7fffffff - 2) / 2 && DSM_MAX_NODES < 0x7fffffff / 64, "the search's pass counter and the wave's node sum fit an int");

}  // namespace ds_mobile
