// diffspectra_amd - colour refinement of molecular graphs, shared by the pair kernels (two molecules at once, one per half wave: PAIR = true;
// k_graph_identity in ds_graph.hip; k_stereo_identity in ds_stereo.hip and k_key_identity in ds_key.hip through ds_sites.h) and ds_smiles.hip
// (one molecule per wave, atoms in lanes 0..28: PAIR = false), and below it the pieces of the individualise-and-refine search that those pair
// kernels run: k_graph_identity's own loop stops at its first leaf, ds_sites::search goes on and tests every leaf against the stereo sites.  The signature and its order are those of
// include/diffspectra_smiles.h: the atom's colour in the top 6 bits (so a round only ever splits classes), below it the commutative sum over
// its bonded neighbours j of fmix(colour_j + 1) * (2 bond_ij + 1), shifted right by 6.
//
// Store: the caller's LDS area with `unsigned long long sig[64], f[64]` and `bonds(side)` = the side's symmetric bond matrix adj[i * 32 + j].
// The pair search asks for more, by name (arrays of 64 are indexed by lane: the generated molecule in lanes 0..28, the ground truth in 32..60):
//   unsigned char adj[2][MA * 32]   both bond matrices, what bonds(side) returns
//   unsigned char stack[MA][64]     colours (ranks below 64) of every open level, before its individualisation
//   int cell[MA], atom[MA], cursor[MA]   per level: the class that is split, its generated atom, the next ground-truth atom to try
//   unsigned char inv[64], img[32]  leaf: ground-truth atom of a colour; image of every generated atom
// Sync: what orders the LDS traffic of the lanes that work on one Store - Block (the workgroup IS the wave pair: the pair kernels) or Wave (several
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

// ---------------------------------------------------------------------------------------------------------------------- the pair search
// Depth-first individualisation over the joint refinement, one wave64 per pair and one wave per workgroup (Block).  The loop that joins the
// pieces stays with the caller (k_graph_identity has the plainest, ds_sites::search the enumerating one), with its own leaf action and its own meaning for the three ways out: per
// pass a leaf test, open_level() if the colouring has cells, next_try(), then "exhausted" (t.w < 0), the budget test, ++used, individualise().
// What the kernels' verdicts lean on is kept true here:
//   a leaf counts only after verify() has compared every label and every bond byte under an explicit bijection;
//   "exhausted" (t.w < 0) means that every ground-truth atom of every open level's class was tried.  The colouring is a deterministic function
//     of the labelled graph that commutes with renaming atoms (each round ranks a signature built from the atom's colour and the multiset of
//     (bond, neighbour colour) jointly over both molecules), so an isomorphism maps every atom to an atom of its own colour: differing
//     histograms (MISMATCH) prove that none exists below a node, and if one exists it sends the individualised atom v to EXACTLY ONE atom w of
//     v's class - the search tries every such w, and below the right w the same argument holds again.  So an exhausted search without a
//     leaf proves that there is no isomorphism, and one that goes on after its leaves meets every isomorphism exactly once;
//   "undecided" means exactly that the budget refused the next try: the test stands after a try was found and before it is spent;
//   the neighbour multiset is hashed (a commutative 64-bit sum): a collision can only leave two atoms in one class that an exact signature
//     would split, which costs search nodes and never a verdict, because nothing above relies on classes being as fine as possible.
// Not shared with k_smiles (ds_smiles.hip), on purpose: that is a one-molecule search with twin pruning, a `tried` mask instead of a second
// side, a certificate comparison at the leaf and Wave ordering; folding it in would need a second axis of templates for four shared lines.

constexpr int FRESH = 63;                 // colour of an individualised atom: ranks stay below 2 * 29 = 58

// Leaf of the search: every colour names one atom per side, which is the only bijection this branch allows.  It is checked in full - it is a
// bijection, same_label(generated slot, ground-truth slot) holds for every atom (the caller's labels: type and charge, ...), and every bond
// byte agrees under it - before anything is called an isomorphism.  Leaves S.img = the map.
template <class Store, class Same>
__device__ bool verify(Store& S, int colour, bool active, int n, int lane, Same same_label) {
  const int idx = lane & 31;
  const bool left = active && lane < 32, right = active && lane >= 32;
  if (right) S.inv[colour] = (unsigned char)idx;
  __syncthreads();
  int m = 0;
  if (left) { m = S.inv[colour] & 31; S.img[idx] = (unsigned char)m; }   // (& 31: an index inside the arrays whatever LDS held)
  __syncthreads();
  bool bad = false;
  if (left) {
    bad = m >= n || !same_label(lane, 32 + m);
    if (!bad)
      for (int j = 0; j < n; ++j) bad |= S.adj[0][j * 32 + idx] != S.adj[1][S.img[j] * 32 + m];
  }
  if (right) {
    int hits = 0;
    for (int j = 0; j < n; ++j) hits += S.img[j] == idx;
    bad = hits != 1;
  }
  __syncthreads();
  return __ballot(bad) == 0ull;
}

// Open level `depth` (< MA: the caller's test) on the lowest class with several atoms: its lowest generated atom will be individualised.
template <class Store>
__device__ __forceinline__ void open_level(Store& S, int& depth, int colour, bool active, int lane, unsigned long long multi) {
  const int side = lane >> 5;
  int c = (active && side == 0 && ((multi >> lane) & 1ull)) ? colour : 64;
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) c = min(c, __shfl_xor(c, o, 64));
  c = ds_rec::uniform_i(c);
  const int v = __ffsll((long long)__ballot(active && side == 0 && colour == c)) - 1;
  S.stack[depth][lane] = (unsigned char)colour;
  if (lane == 0) { S.cell[depth] = c; S.atom[depth] = v; S.cursor[depth] = 0; }
  __syncthreads();
  ++depth;
}

struct Try { int v, w; };                 // generated atom and ground-truth atom to individualise; w < 0: nothing left to try anywhere

// The next untried ground-truth atom of the deepest level that has one; levels without are closed.  Leaves `colour` = that level's colouring.
template <class Store>
__device__ __forceinline__ Try next_try(Store& S, int& depth, int& colour, bool active, int lane) {
  const int idx = lane & 31, side = lane >> 5;
  Try t = {-1, -1};
  while (depth > 0) {                     // at most 29 levels
    const int f = depth - 1;
    const int c = ds_rec::uniform_i(S.cell[f]), from = ds_rec::uniform_i(S.cursor[f]);
    colour = S.stack[f][lane];
    const unsigned long long cand = __ballot(active && side == 1 && colour == c && idx >= from);
    if (cand) { t.v = ds_rec::uniform_i(S.atom[f]); t.w = __ffsll((long long)cand) - 1 - 32; break; }
    --depth;
  }
  return t;
}

// Spend the try: move the level's cursor past w, give v and w the fresh colour and refine.  Returns refine()'s state.
template <class Store>
__device__ __forceinline__ int individualise(Store& S, int depth, Try t, int& colour, bool active, int n, int lane, unsigned long long& multi) {
  __syncthreads();                        // every lane has read the level's cursor
  if (lane == 0) S.cursor[depth - 1] = t.w + 1;
  if (active && (lane == t.v || lane == 32 + t.w)) colour = FRESH;
  __syncthreads();
  return refine<true>(S, colour, active, n, lane, multi, Block{});
}

}  // namespace ds_refine
