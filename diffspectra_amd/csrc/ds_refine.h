// diffspectra_amd - colour refinement of molecular graphs, shared by ds_graph.hip (two molecules at once, one per half wave: PAIR = true) and
// ds_smiles.hip (one molecule per wave, atoms in lanes 0..28: PAIR = false).  The signature and its order are those of
// include/diffspectra_smiles.h: the atom's colour in the top 6 bits (so a round only ever splits classes), below it the commutative sum over
// its bonded neighbours j of fmix(colour_j + 1) * (2 bond_ij + 1), shifted right by 6.
//
// Store: the caller's LDS area with `unsigned long long sig[64], f[64]` and `bonds(side)` = the side's symmetric bond matrix adj[i * 32 + j].
// Sync: what orders the LDS traffic of the lanes that work on one Store - Block (the workgroup IS the wave pair: ds_graph.hip) or Wave (several
// waves per workgroup, each on its own Store, inside loops whose trip counts differ from wave to wave: no workgroup barrier may stand there).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ds_records.h"

namespace ds_refine {

struct Block {
  __device__ __forceinline__ void operator()() const { __syncthreads(); }
};

// The LDS operations of one wave are issued and served in order; what is left to do is to keep the compiler from moving or merging accesses
// across the point where other lanes' writes are read: the fences of __syncthreads() around a barrier that costs nothing.
struct Wave {
  __device__ __forceinline__ void operator()() const {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  }
};

struct Ranked { int colour, eq_g, eq_r; bool leader; };

// Rank of `sig` over the active atoms: colour = atoms with a smaller signature (ties share a colour); eq_g / eq_r = atoms of the generated /
// ground-truth side with this signature (PAIR = false: eq_g counts the molecule's atoms, eq_r stays 0); leader = no lower atom of the own side
// has it.  PAIR = true ranks jointly over both sides; every lane's `sig` is stored.  PAIR = false: lanes 0..31 store theirs, and an atom that
// takes no part passes ~0, which is above every signature.
template <bool PAIR, class Store, class Sync>
__device__ __forceinline__ Ranked rank_jointly(Store& S, unsigned long long sig, int n, int lane, Sync sync) {
  const int idx = lane & 31;
  const bool right = PAIR && lane >= 32;
  if (PAIR || lane < 32) S.sig[lane] = sig;
  sync();
  Ranked r = {0, 0, 0, true};
  for (int k = 0; k < n; ++k) {
    const unsigned long long a = S.sig[k];
    if constexpr (PAIR) {
      const unsigned long long b = S.sig[32 + k];
      r.colour += (a < sig) + (b < sig);
      r.eq_g += a == sig;
      r.eq_r += b == sig;
      if (k < idx && (right ? b : a) == sig) r.leader = false;
    } else {
      r.colour += a < sig;
      r.eq_g += a == sig;
      if (k < idx && a == sig) r.leader = false;
    }
  }
  sync();
  return r;
}

enum { MISMATCH = 0, DISCRETE = 1, CELLS = 2 };

// Colour refinement to the stable colouring.  At most n + 1 rounds: every round but the last adds a class and there are at most n.
// PAIR = true: both molecules at once; returns MISMATCH as soon as the sides' histograms differ, else DISCRETE (every class one atom per
// side) or CELLS with `multi` = the generated atoms that share their class.  PAIR = false: `active` names the atoms that take part (lanes
// 0..28 at most), the bond bytes of every other atom < n are 0; never MISMATCH, `multi` = the atoms that share their class.
template <bool PAIR, class Store, class Sync>
__device__ __forceinline__ int refine(Store& S, int& colour, bool active, int n, int lane, unsigned long long& multi, Sync sync) {
  const int idx = lane & 31, side = PAIR ? lane >> 5 : 0;
  const unsigned char* __restrict__ adj = S.bonds(side);
  int classes = 0;
  multi = 0ull;
  for (int round = 0; round <= n; ++round) {
    if (PAIR || lane < 32) S.f[lane] = ds_rec::fmix((unsigned long long)colour + 1ull);
    sync();
    unsigned long long acc = 0ull;
    if (active)
      for (int j = 0; j < n; ++j) {
        const unsigned b = adj[j * 32 + idx];
        if (b) acc += S.f[side * 32 + j] * (unsigned long long)(2u * b + 1u);
      }
    const unsigned long long sig = ((unsigned long long)colour << 58) | (acc >> 6);
    const Ranked r = rank_jointly<PAIR>(S, PAIR || active ? sig : ~0ull, n, lane, sync);
    if (active) colour = r.colour;
    if (PAIR && __ballot(active && r.eq_g != r.eq_r) != 0ull) return MISMATCH;
    const int now = __popcll(__ballot(active && side == 0 && r.leader));
    multi = __ballot(active && side == 0 && r.eq_g > 1);
    if (now == classes) break;
    classes = now;
  }
  return multi ? CELLS : DISCRETE;
}

}  // namespace ds_refine
