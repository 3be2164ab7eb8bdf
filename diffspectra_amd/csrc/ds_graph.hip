// diffspectra_amd - molecular-graph identity of the evaluation path: is the generated molecule THE ground-truth molecule (same labelled graph:
// atom type, formal charge, bond order), whatever its conformation, and a permutation-invariant hash per molecule.  One wave64 per pair /
// per molecule, integers only, no atomics (ds_graph_identity_records and ds_graph_hash_records in include/diffspectra_hip.h state the
// semantics and the exact hash formula; DESIGN.md section 10 has the algorithm and the figures).
//
// k_graph_identity runs the pair search of ds_refine.h, where the argument for its verdicts stands above the code it describes.  What this
// file adds to it: the labels are atom type and formal charge; verdict 1 is written only after ds_refine::verify() has compared every type,
// charge and bond byte under an explicit bijection; verdict 0 is written only (a) for unequal atom counts, (b) when the ROOT colouring's
// histograms differ, or (c) when the search below the root is exhausted; a search the budget stops is verdict 2.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/diffspectra_hip.h"
#include "ds_records.h"
#include "ds_refine.h"
#include "ds_host.h"   // DST_CHECK_LAUNCH

namespace {

using ds_rec::MA;                         // 29 atoms: lanes 0..28 hold the generated molecule, lanes 32..60 the ground truth
using ds_rec::fmix;                       // the 64-bit finaliser and the pair mix of the header's hash formula
using ds_rec::mix2;
constexpr unsigned ALL = ~0u;             // keep mask of ds_rec::load_bonds: every atom (the kernels below mask by n where they read)

struct Pair {                             // both molecules of a pair in LDS; arrays of 64 are indexed by lane
  unsigned char adj[2][MA * 32];
  unsigned char type[64], fc[64];
  unsigned long long sig[64], f[64];      // signatures being ranked; per-atom colour hash of the running round
  unsigned char stack[MA][64];            // the pair search's fields, as ds_refine.h names them
  int cell[MA], atom[MA], cursor[MA];
  unsigned char inv[64], img[32];
  __device__ __forceinline__ const unsigned char* bonds(int side) const { return adj[side]; }
};

using ds_refine::Ranked;                  // the joint ranking and the refinement of both molecules at once: ds_refine.h, PAIR = true
using ds_refine::MISMATCH;
using ds_refine::DISCRETE;
using ds_refine::CELLS;
constexpr ds_refine::Block SYNC{};        // one wave per workgroup: the workgroup barrier orders the pair's LDS traffic

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
      const Ranked first = ds_refine::rank_jointly<true>(S, (unsigned long long)(type << 8 | fc), n, lane, SYNC);
      int colour = active ? first.colour : 0;
      unsigned long long multi = 0ull;
      int st = __ballot(active && first.eq_g != first.eq_r) ? MISMATCH : ds_refine::refine<true>(S, colour, active, n, lane, multi, SYNC);
      int depth = 0;                                         // open levels: S.stack[0 .. depth-1]
      const auto same_label = [](int a, int b) { return S.type[a] == S.type[b] && S.fc[a] == S.fc[b]; };
      out = DS_GRAPH_UNDECIDED;
      for (int it = 0; it <= max_nodes; ++it) {              // every pass but the last spends one search node
        if (st == DISCRETE && ds_refine::verify(S, colour, active, n, lane, same_label)) { out = DS_GRAPH_IDENTICAL; break; }
        if (st == CELLS) {
          if (depth >= MA) break;                            // (cannot happen: every level makes one more generated atom a class of its own)
          ds_refine::open_level(S, depth, colour, active, lane, multi);
        }
        const ds_refine::Try t = ds_refine::next_try(S, depth, colour, active, lane);
        if (t.w < 0) { out = DS_GRAPH_DIFFERENT; break; }    // nothing left to try anywhere: the root is dead
        if (used >= max_nodes) break;                        // the budget does not cover this try: undecided
        ++used;
        st = ds_refine::individualise(S, depth, t, colour, active, n, lane, multi);
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
