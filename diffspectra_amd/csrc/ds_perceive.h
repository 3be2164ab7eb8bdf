// diffspectra_amd - perception of one result record by one wave64, an atom per lane: what the per-record evaluation kernels share
// (ds_valence.hip, ds_groups.hip, ds_scaffold.hip, ds_smiles.hip, ds_substructure.hip, ds_brics.hip, ds_mobile.hip, ds_fraggle.hip).  The
// definitions are those of the public headers: applied charges and the valence check in include/diffspectra_valence.h, ring bonds and the
// candidate / electron rule in
// include/diffspectra_groups.h, the plain-hydrogen fold in include/diffspectra_smiles.h, the matched graph in
// include/diffspectra_substructure.h.  Everything here is inlined into its caller, which keeps its own LDS struct and passes the arrays: a
// result that a caller does not read costs it nothing.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ds_bonds.h"
#include "ds_records.h"
#include "ds_refine.h"   // the barrier objects: ds_refine::Block, ds_refine::Wave

namespace ds_perceive {

using ds_rec::MA;
using ds_rec::uniform_i;
constexpr unsigned ALL = ~0u;             // keep mask of ds_rec::load_bonds: every atom (the rows are read up to n only)
constexpr int MAX_ORDER = 3, MAX_TYPE = 4;
constexpr int H = 0, C = 1, N = 2, O = 3, F = 4;
constexpr unsigned NONE = 3u;             // electron code of "no candidate"; the counts are 0, 1, 2
constexpr int NO_PARTNER = 31;            // a bit no member mask holds: an atom without a double bond reads its "outside" count, which equals the other

__device__ __forceinline__ unsigned low32(unsigned long long ballot) { return (unsigned)ballot; }   // atoms live in lanes 0..28

// OR, sum, minimum and maximum over the 64 lanes, as wave-uniform values
__device__ __forceinline__ unsigned wave_or(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v |= (unsigned)__shfl_xor((int)v, o, 64);
  return (unsigned)uniform_i((int)v);
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return uniform_i(v);
}
__device__ __forceinline__ unsigned wave_min(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, (unsigned)__shfl_xor((int)v, o, 64));
  return (unsigned)uniform_i((int)v);
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return uniform_i(v);
}

struct Atom {                             // what a lane knows of its atom once the record is read
  bool active, bad;                       // lane < n; its type is above MAX_TYPE or one of its orders above MAX_ORDER
  int type, raw, val;                     // type byte, charge byte (signed), valence = sum of the orders
  unsigned nb, nb1, nb2, nb3;             // bit j = bonded to atom j by any order / by order 1 / 2 / 3
};

// Reads record `mine` (not touched when n = 0: a wave without a record passes n = 0) and leaves the orders among atoms < n in adj.  Holds the
// one barrier between writing and reading adj: Block where every wave of the workgroup comes here, Wave where a wave is on its own.
template <class Sync>
__device__ __forceinline__ Atom scan(unsigned char* __restrict__ adj, const unsigned char* __restrict__ mine, int n, int lane, Sync sync) {
  Atom A = {lane < n, false, 0, 0, 0, 0u, 0u, 0u, 0u};
  if (A.active) {
    A.type = mine[DS_REC_TYPE + lane];
    A.raw = (int)(signed char)mine[DS_REC_FC + lane];
  }
  bool bad = A.type > MAX_TYPE;
  if (n > 0) ds_rec::load_bonds(adj, mine, ALL, lane);
  sync();
  if (A.active)
    for (int j = 0; j < n; ++j) {
      const unsigned b = adj[lane * 32 + j];
      bad |= b > (unsigned)MAX_ORDER;
      A.val += (int)b;
      A.nb |= (b ? 1u : 0u) << j;
      A.nb1 |= (b == 1u ? 1u : 0u) << j;
      A.nb2 |= (b == 2u ? 1u : 0u) << j;
      A.nb3 |= (b == 3u ? 1u : 0u) << j;
    }
  A.bad = bad;
  return A;
}

// A record is usable if it has atoms and none of them is bad: wave-uniform, asked by the whole wave.  Apart from scan, so that
// ds_valence.hip asks once behind its two ways of reading the atoms (a ballot in each branch costs its kernels four SGPRs); in scan `bad`
// is a local that is stored once: accumulated in the struct inside the loop it leaves the SGPR masks for a VGPR.
__device__ __forceinline__ bool usable_record(const Atom& A, int n) { return n > 0 && __ballot(A.active && A.bad) == 0ull; }

// t = min(type, MAX_TYPE): a table index whatever the byte.  atom_fc_num: N+1, N-1, C+1, O-1, C-1
__device__ __forceinline__ int applied_charge(int t, int raw) {
  return ((t == C || t == N) && (raw == 1 || raw == -1)) || (t == O && raw == -1) ? raw : 0;
}
__device__ __forceinline__ int max_valence(int t, int q) { return ds_bonds::c_valence[t] + (t == C ? -abs(q) : (t == N || t == O) ? q : 0); }

// A hydrogen that is written into its neighbour: no charge, one bond, to an atom that is no hydrogen - and that bond of order 1, which the
// caller tests last, from what it holds (the bond byte in LDS, or the order-1 mask).
__device__ __forceinline__ bool plain_hydrogen(bool on, int t, int raw, unsigned nb, unsigned hydrogens) {
  return on && t == H && raw == 0 && __popc(nb) == 1 && !(nb & hydrogens);
}

// Components: comp = the atoms known to be connected to this one (itself and its neighbours to begin with, 0 for a lane that takes no part);
// a round ORs in what they know, so the reach doubles.  Called by the whole wave.
__device__ __forceinline__ unsigned components(unsigned comp, int n) {
  for (int reach = 1; reach < n; reach <<= 1) {
    unsigned next = comp;
    for (int j = 0; j < n; ++j) {
      const unsigned cj = (unsigned)__shfl((int)comp, j, 64);
      if ((comp >> j) & 1u) next |= cj;
    }
    const bool grew = __ballot(next != comp) != 0ull;
    comp = next;
    if (!grew) break;
  }
  return comp;
}

// `reached` grown over the neighbour words nbr[] in LDS until it holds `goal` or nothing is left: `todo` = the atoms of `reached` still to be
// expanded; every atom is expanded at most once.  Read inside divergent code, so LDS and no shuffles.
__device__ __forceinline__ unsigned reach(const unsigned (&nbr)[32], unsigned reached, unsigned todo, unsigned goal) {
  while (todo && !(reached & goal)) {
    const int j = __ffs((int)todo) - 1;
    todo &= todo - 1u;
    const unsigned fresh = nbr[j] & ~reached;
    reached |= fresh;
    todo |= fresh;
  }
  return reached;
}

// Is the bond of atom `me` (neighbours nb) to its neighbour `goal` a ring bond: goal is reached without it, goal itself is never expanded
__device__ __forceinline__ bool ring_bond(const unsigned (&nbr)[32], unsigned me, unsigned nb, unsigned goal) {
  return (reach(nbr, me | (nb & ~goal), nb & ~goal, goal) & goal) != 0u;
}

// The candidate / electron rule.  electron_rule gives what does not depend on the cycle; for an atom with a double bond (partner !=
// NO_PARTNER) the count with the partner outside the cycle is still open, and double_bond_outside closes it once the caller knows whether
// that bond is a ring bond.  isNO = the N and O atoms of the record.
struct Electrons {
  unsigned e_in, e_out;                   // count with the partner inside the cycle / outside it, NONE = no candidate
  int partner;
  __device__ __forceinline__ unsigned word() const { return e_in | (e_out << 2) | ((unsigned)partner << 4); }   // what six_electrons reads
};

__device__ __forceinline__ Electrons electron_rule(bool on, int t, int q, int X, int dbl, int trp, unsigned nb2) {
  Electrons e = {NONE, NONE, NO_PARTNER};
  if (on && trp == 0 && dbl <= 1 && X <= 3) {
    if (dbl == 1) {
      if ((t == C && X == 3 && q == 0) || (t == N && ((X == 2 && q == 0) || (X == 3 && q == 1)))) {
        e.e_in = 1u;
        e.partner = __ffs((int)nb2) - 1;
      }
    } else if (t == C) {
      if (X == 3 && q == -1) e.e_in = e.e_out = 2u;
      else if (X == 3 && q == 1) e.e_in = e.e_out = 0u;
    } else if (t == N) {
      if ((X == 3 && q == 0) || (X == 2 && q == -1)) e.e_in = e.e_out = 2u;
    } else if (t == O) {
      if (X == 2 && q == 0) e.e_in = e.e_out = 2u;
    }
  }
  return e;
}
__device__ __forceinline__ unsigned double_bond_outside(bool ring, int partner, unsigned isNO) { return ring ? 1u : ((isNO >> partner) & 1u) ? 0u : NONE; }

// Is the cycle with the member mask `members` aromatic: every member a candidate for it, six electrons in all.
__device__ __forceinline__ bool six_electrons(const unsigned (&electrons)[32], unsigned members) {
  unsigned sum = 0u;
  bool all = true;
  for (unsigned m = members; m; m &= m - 1u) {                                   // 5 or 6 members
    const unsigned w = electrons[__ffs((int)m) - 1];
    const unsigned e = ((members >> (w >> 4)) & 1u) ? (w & 3u) : ((w >> 2) & 3u);
    all &= e != NONE;
    sum += e;
  }
  return all && sum == 6u;
}

// The aromatic cycles of 5 and 6 atoms through atom `me` (a candidate, neighbours nb) over `candidates`: LOWEST = only those it is the lowest
// atom of.  Candidates have at most three neighbours, so 3 * 2 * 2 * 2 * 2 partial paths at the most; a cycle is met in both directions and
// taken in the one whose last atom is above its second.  closed(members, second atom, last atom) is called for each.
template <bool LOWEST, class Closed>
__device__ __forceinline__ void aromatic_cycles(const unsigned (&any)[32], const unsigned (&electrons)[32], unsigned me, unsigned nb, unsigned candidates,
                                                Closed closed) {
  const unsigned open = candidates & ~(LOWEST ? (me << 1) - 1u : me);
  for (unsigned c1 = nb & open; c1; c1 &= c1 - 1u) {
    const int a1 = __ffs((int)c1) - 1;
    const unsigned m1 = me | (1u << a1);
    for (unsigned c2 = any[a1] & open & ~m1; c2; c2 &= c2 - 1u) {
      const int a2 = __ffs((int)c2) - 1;
      const unsigned m2 = m1 | (1u << a2);
      for (unsigned c3 = any[a2] & open & ~m2; c3; c3 &= c3 - 1u) {
        const int a3 = __ffs((int)c3) - 1;
        const unsigned m3 = m2 | (1u << a3);
        for (unsigned c4 = any[a3] & open & ~m3; c4; c4 &= c4 - 1u) {
          const int a4 = __ffs((int)c4) - 1;
          const unsigned m4 = m3 | (1u << a4), n4 = any[a4];
          if ((n4 & me) && a4 > a1 && six_electrons(electrons, m4)) closed(m4, a1, a4);
          for (unsigned c5 = n4 & open & ~m4; c5; c5 &= c5 - 1u) {
            const int a5 = __ffs((int)c5) - 1;
            const unsigned m5 = m4 | (1u << a5);
            if ((any[a5] & me) && a5 > a1 && six_electrons(electrons, m5)) closed(m5, a1, a5);
          }
        }
      }
    }
  }
}

// The matched graph of include/diffspectra_substructure.h as one lane sees it, for the kernels that run on it (ds_substructure.hip,
// ds_brics.hip): the fold, the ring bonds of every bond and the aromatic-bond neighbours from the cycles through the lane's OWN atom (not only
// those it is the lowest atom of), so that a lane learns them without a scatter.  From these a caller forms the bond classes of its atom:
// kind single / double / triple = nb1 / nb2 / nb3 without arom_nb, aromatic = arom_nb, each among `matchable`, by ring = ring_nb.
struct Matched {
  bool usable, on, node;                  // the record is usable / and this lane holds an atom / and that atom is matchable
  int t, q, hi;                           // type (a table index), applied charge, implicit hydrogens
  unsigned nb, nb1, nb2, nb3;             // bonded by any order / by order 1 / 2 / 3; 0 in an unusable record
  unsigned isH, isN, isO;                 // the atoms of these elements
  unsigned matchable, ring_nb, arom_nb;   // matchable atoms (wave-uniform); the neighbours over a ring bond, over an aromatic bond
};

// Holds three workgroup barriers, which every wave of the workgroup reaches.  n = 0: a wave without a record; `mine` is not touched.  Leaves
// adj, any (neighbours by any order), matched (the same among matchable atoms, 0 for a folded hydrogen) and the electron words in the
// caller's LDS.  closed(members) is called for every aromatic cycle through the lane's atom.
template <class Closed>
__device__ __forceinline__ Matched matched_graph(unsigned char* __restrict__ adj, unsigned (&any)[32], unsigned (&matched)[32], unsigned (&electrons)[32],
                                                 const unsigned char* __restrict__ mine, int n, int lane, Closed closed) {
  const Atom A = scan(adj, mine, n, lane, ds_refine::Block{});
  const bool usable = usable_record(A, n), on = usable && A.active;
  const int t = min(A.type, MAX_TYPE);
  // an unusable record has no atoms from here on
  const unsigned nb = on ? A.nb : 0u, nb1 = on ? A.nb1 : 0u, nb2 = on ? A.nb2 : 0u, nb3 = on ? A.nb3 : 0u;

  const unsigned isH = low32(__ballot(on && t == H)), isN = low32(__ballot(on && t == N)), isO = low32(__ballot(on && t == O));
  const int q = applied_charge(t, A.raw);
  const int hi = max(0, max_valence(t, q) - A.val);
  const int dbl = __popc(nb2), trp = __popc(nb3);
  const int X = __popc(nb) + hi;
  const unsigned matchable = low32(__ballot(on && !(plain_hydrogen(on, t, A.raw, nb, isH) && nb1 == nb)));
  const unsigned me = lane < 32 ? 1u << lane : 0u;
  const bool node = (matchable & me) != 0u;
  if (lane < 32) {
    any[lane] = nb;
    matched[lane] = node ? nb & matchable : 0u;
  }
  __syncthreads();

  // ring bonds: neighbour j is reached without the bond to it; every atom is expanded once per neighbour
  unsigned ring_nb = 0u;
  for (unsigned left = nb; left; left &= left - 1u) {
    const unsigned goal = left & (0u - left);
    if (ring_bond(any, me, nb, goal)) ring_nb |= goal;
  }
  Electrons e = electron_rule(on, t, q, X, dbl, trp, nb2);
  if (e.partner != NO_PARTNER) e.e_out = double_bond_outside((ring_nb & nb2) != 0u, e.partner, isN | isO);
  if (lane < 32) electrons[lane] = e.word();
  __syncthreads();
  const unsigned candidates = low32(__ballot(e.e_in != NONE));

  unsigned arom_nb = 0u;
  if (e.e_in != NONE)
    aromatic_cycles<false>(any, electrons, me, nb, candidates, [&](unsigned members, int second, int last) {
      arom_nb |= (1u << second) | (1u << last);
      closed(members);
    });
  return {usable, on, node, t, q, hi, nb, nb1, nb2, nb3, isH, isN, isO, usable ? matchable : 0u, ring_nb, arom_nb};
}

static_assert(MA <= 29, "an atom mask fits a 32-bit word with lanes 29..31 clear; a partner index fits the electron word");

}  // namespace ds_perceive
