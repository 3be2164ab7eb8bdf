// diffspectra_amd - molecular-graph identity of the evaluation path: is the generated molecule THE ground-truth molecule (same labelled graph:
// atom type, formal charge, bond order), whatever its conformation, and a permutation-invariant hash per molecule.  One wave64 per pair /
// per molecule, integers only, no atomics (ds_graph_identity_records and ds_graph_hash_records in include/diffspectra_hip.h state the
// semantics and the exact hash formula; DESIGN.md section 10 has the algorithm and the figures).
//
// Soundness of k_graph_identity, in two lines that the code below keeps true:
//   verdict 1 is written only after verify() has compared every type, charge and bond byte under an explicit bijection;
//   verdict 0 is written only (a) for unequal atom counts, (b) when the ROOT colouring's histograms differ, or (c) when the search below the
//     root is exhausted.  The colouring is a deterministic function of the labelled graph that commutes with renaming atoms (each round
//     ranks a signature built from the atom's colour and the multiset of (bond, neighbour colour) jointly over both molecules), so an
//     isomorphism maps every atom to an atom of its own colour: differing histograms prove that none exists, and if one exists it sends the
//     individualised atom v to SOME atom w of v's class - the search tries every such w, and below the right w the same argument holds
//     again, so an exhausted search proves that none exists.  The neighbour multiset is hashed (a commutative 64-bit sum): a collision can
//     only leave two atoms in one class that an exact signature would split, which costs search nodes and never a wrong verdict, because
//     neither (1) nor (0) relies on classes being as fine as possible.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/diffspectra_hip.h"
#include "ds_records.h"
#include "ds_refine.h"
#include "ds_host.h"   // DST_CHECK_LAUNCH

namespace {

using ds_rec::MA;                         // 29 atoms: lanes 0..28 hold the generated molecule, lanes 32..60 the ground truth
using ds_rec::uniform_i;
using ds_rec::fmix;                       // the 64-bit finaliser and the pair mix of the header's hash formula
using ds_rec::mix2;
constexpr int FRESH = 63;                 // colour of an individualised atom: ranks stay below 2 * 29 = 58
constexpr unsigned ALL = ~0u;             // keep mask of ds_rec::load_bonds: every atom (the kernels below mask by n where they read)


struct Pair {                             // both molecules of a pair in LDS; arrays of 64 are indexed by lane
  unsigned char adj[2][MA * 32];
  unsigned char type[64], fc[64];
  unsigned long long sig[64], f[64];      // signatures being ranked; per-atom colour hash of the running round
  unsigned char stack[MA][64];            // colours (ranks below 64) of every open level of the search, before its individualisation
  int cell[MA], atom[MA], cursor[MA];     // per level: the class that is split, its generated atom, the next ground-truth atom to try
  unsigned char inv[64], img[32];         // leaf: ground-truth atom of a colour; image of every generated atom
  __device__ __forceinline__ const unsigned char* bonds(int side) const { return adj[side]; }
};

using ds_refine::Ranked;                  // the joint ranking and the refinement of both molecules at once: ds_refine.h, PAIR = true
using ds_refine::MISMATCH;
using ds_refine::DISCRETE;
using ds_refine::CELLS;
constexpr ds_refine::Block SYNC{};        // one wave per workgroup: the workgroup barrier orders the pair's LDS traffic

__device__ __forceinline__ Ranked rank_jointly(Pair& S, unsigned long long sig, int n, int lane) {
  return ds_refine::rank_jointly<true>(S, sig, n, lane, SYNC);
}
__device__ __forceinline__ int refine(Pair& S, int& colour, bool active, int n, int lane, unsigned long long& multi) {
  return ds_refine::refine<true>(S, colour, active, n, lane, multi, SYNC);
}

// Leaf of the search: every colour names one atom per side, which is the only bijection this branch allows.  It is checked in full - it is a
// bijection, and every type, charge and bond byte agrees under it - before anything is called identical.  Leaves S.img = the map.
__device__ bool verify(Pair& S, int colour, bool active, int n, int lane) {
  const int idx = lane & 31;
  const bool left = active && lane < 32, right = active && lane >= 32;
  if (right) S.inv[colour] = (unsigned char)idx;
  __syncthreads();
  int m = 0;
  if (left) { m = S.inv[colour] & 31; S.img[idx] = (unsigned char)m; }   // (& 31: an index inside the arrays whatever LDS held)
  __syncthreads();
  bool bad = false;
  if (left) {
    bad = m >= n || S.type[lane] != S.type[32 + m] || S.fc[lane] != S.fc[32 + m];
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

__global__ __launch_bounds__(64) void k_graph_identity(const unsigned char* __restrict__ prb_rec, const int32_t* __restrict__ prb_n,
                                                       const unsigned char* __restrict__ ref_rec, const int32_t* __restrict__ ref_n,
                                                       const int64_t* __restrict__ ref_index, int64_t M, int max_nodes,
                                                       unsigned char* __restrict__ verdict, int32_t* __restrict__ nodes, int32_t* __restrict__ map) {
  __shared__ Pair S;
  const int64_t p = blockIdx.x;
  const int lane = threadIdx.x, idx = lane & 31, side = lane >> 5;
  const ds_rec::Pair q = ds_rec::pair_of(p, prb_rec, prb_n, ref_rec, ref_n, ref_index, M);
  int out = DS_GRAPH_INVALID, used = 0;
  if (q.valid) {
    const int ng = q.n_prb(), nr = q.n_ref();
    const unsigned char* __restrict__ mine = side ? q.ref : q.prb;
    out = DS_GRAPH_DIFFERENT;
    if (ng == nr) {
      const int n = ng;
      const bool active = idx < n;
      ds_rec::load_bonds(S.adj[0], q.prb, ALL, lane);
      ds_rec::load_bonds(S.adj[1], q.ref, ALL, lane);
      const unsigned type = active ? mine[DS_REC_TYPE + idx] : 0u, fc = active ? mine[DS_REC_FC + idx] : 0u;
      S.type[lane] = (unsigned char)type;
      S.fc[lane] = (unsigned char)fc;
      __syncthreads();
      // initial colour: (type, charge) ranked jointly
      const Ranked first = rank_jointly(S, (unsigned long long)(type << 8 | fc), n, lane);
      int colour = active ? first.colour : 0;
      unsigned long long multi = 0ull;
      int st = __ballot(active && first.eq_g != first.eq_r) ? MISMATCH : refine(S, colour, active, n, lane, multi);
      int depth = 0;                                         // open levels: S.stack[0 .. depth-1]
      out = DS_GRAPH_UNDECIDED;
      for (int it = 0; it <= max_nodes; ++it) {              // every pass but the last spends one search node
        if (st == DISCRETE && verify(S, colour, active, n, lane)) { out = DS_GRAPH_IDENTICAL; break; }
        if (st == CELLS) {
          if (depth >= MA) break;                            // (cannot happen: every level makes one more generated atom a class of its own)
          // open a level on the lowest class with several atoms: its lowest generated atom will be individualised
          int c = (active && side == 0 && ((multi >> lane) & 1ull)) ? colour : 64;
#pragma unroll
          for (int o = 16; o > 0; o >>= 1) c = min(c, __shfl_xor(c, o, 64));
          c = uniform_i(c);
          const int v = __ffsll((long long)__ballot(active && side == 0 && colour == c)) - 1;
          S.stack[depth][lane] = (unsigned char)colour;
          if (lane == 0) { S.cell[depth] = c; S.atom[depth] = v; S.cursor[depth] = 0; }
          __syncthreads();
          ++depth;
        }
        // the next untried ground-truth atom of the deepest level that has one; levels without are closed
        int v = -1, w = -1;
        while (depth > 0) {                                  // at most 29 levels
          const int f = depth - 1;
          const int c = uniform_i(S.cell[f]), from = uniform_i(S.cursor[f]);
          colour = S.stack[f][lane];
          const unsigned long long cand = __ballot(active && side == 1 && colour == c && idx >= from);
          if (cand) { v = uniform_i(S.atom[f]); w = __ffsll((long long)cand) - 1 - 32; break; }
          --depth;
        }
        if (w < 0) { out = DS_GRAPH_DIFFERENT; break; }      // nothing left to try anywhere: the root is dead
        if (used >= max_nodes) break;                        // the budget does not cover this try: undecided
        ++used;
        __syncthreads();                                     // every lane has read the level's cursor
        if (lane == 0) S.cursor[depth - 1] = w + 1;
        if (active && (lane == v || lane == 32 + w)) colour = FRESH;
        __syncthreads();
        st = refine(S, colour, active, n, lane, multi);
      }
      if (out == DS_GRAPH_IDENTICAL && lane < n) map[p * MA + lane] = S.img[lane];
      if (out == DS_GRAPH_IDENTICAL && lane >= n && lane < MA) map[p * MA + lane] = -1;
    }
  }
  if (out != DS_GRAPH_IDENTICAL && lane < MA) map[p * MA + lane] = -1;
  if (lane == 0) {
    verdict[p] = (unsigned char)out;
    nodes[p] = used;
  }
}

struct Molecule {
  unsigned char adj[MA * 32];
  unsigned long long h[32];
};

// the hash of the header, term for term: lanes 0..28 are atoms
__global__ __launch_bounds__(64) void k_graph_hash(const unsigned char* __restrict__ rec, const int32_t* __restrict__ n_atoms,
                                                   unsigned long long* __restrict__ hash) {
  __shared__ Molecule S;
  const int64_t p = blockIdx.x;
  const int lane = threadIdx.x;
  const int n = ds_rec::atoms_of(n_atoms, p);
  const unsigned char* __restrict__ mine = rec + p * DS_RECORD_BYTES;
  const bool active = lane < n;
  ds_rec::load_bonds(S.adj, mine, ALL, lane);
  unsigned long long h = active ? mix2(mine[DS_REC_TYPE + lane], mine[DS_REC_FC + lane]) : 0ull;
  for (int round = 0; round < MA; ++round) {
    if (lane < 32) S.h[lane] = h;
    __syncthreads();
    unsigned long long acc = 0ull;
    if (active)
      for (int j = 0; j < n; ++j) {
        const unsigned b = S.adj[j * 32 + lane];
        if (b) acc += mix2(S.h[j], b);
      }
    __syncthreads();
    if (active) h = mix2(h, acc);
  }
  if (lane < 32) S.h[lane] = fmix(h);
  __syncthreads();
  if (lane == 0) {
    unsigned long long total = 0ull;
    for (int j = 0; j < n; ++j) total += S.h[j];
    hash[p] = mix2((unsigned long long)n, total);
  }
}

}  // namespace

extern "C" int ds_graph_identity_records(const uint8_t* prb_rec, const int32_t* prb_n, int64_t P, const uint8_t* ref_rec, const int32_t* ref_n,
                                         int64_t M, const int64_t* ref_index, int32_t max_nodes, uint8_t* verdict, int32_t* nodes, int32_t* map,
                                         void* stream) {
  const int go = ds_rec::check_pairs(max_nodes >= 0 && max_nodes <= DS_GRAPH_MAX_NODES, P, M, prb_rec, prb_n, ref_rec, ref_n, ref_index,
                                     {verdict, nodes, map});
  if (go != ds_rec::LAUNCH) return go;
  hipLaunchKernelGGL(k_graph_identity, dim3((unsigned)P), dim3(64), 0, (hipStream_t)stream, prb_rec, prb_n, ref_rec, ref_n, ref_index, M,
                     (int)max_nodes, verdict, nodes, map);
  return DST_CHECK_LAUNCH();
}

extern "C" int ds_graph_hash_records(const uint8_t* rec, const int32_t* n, int64_t P, uint64_t* hash, void* stream) {
  const int go = ds_rec::check_table(true, P, rec, n, {hash});
  if (go != ds_rec::LAUNCH) return go;
  hipLaunchKernelGGL(k_graph_hash, dim3((unsigned)P), dim3(64), 0, (hipStream_t)stream, rec, n, reinterpret_cast<unsigned long long*>(hash));
  return DST_CHECK_LAUNCH();
}
