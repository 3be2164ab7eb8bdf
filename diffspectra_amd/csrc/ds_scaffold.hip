// diffspectra_amd - scaffold analytics on result records: the Bemis-Murcko scaffold atoms (the 2-core of the heavy graph plus its exocyclic
// atoms), the ring atoms and the ring count behind the "Scaf" number of the reference's set metrics.  include/diffspectra_scaffold.h states
// every definition (heavy graph, core, exocyclic atoms, ring bonds, the cyclomatic ring count, the unusable rule); DESIGN.md section 18 has
// the method and the round bound.
//
// One wave64 per record, DSK_WAVES records per workgroup, an atom per lane.  LDS holds, per wave, the bond matrix of ds_rec::load_bonds and one
// word per atom: its neighbours inside the core.  The pruning and the component growth are wave-wide (ballots, shuffles) and run outside
// divergent code; a lane's ring-bond tests read other atoms' words inside divergent loops, so they read LDS and never shuffle.  Integers
// only, no atomics, no early exit: a wave without a record takes part in the workgroup's barriers and writes nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/diffspectra_scaffold.h"
#include "ds_records.h"
#include "ds_host.h"   // DST_CHECK_LAUNCH

namespace {

using ds_rec::MA;
using ds_rec::uniform_i;
constexpr unsigned ALL = ~0u;             // keep mask of ds_rec::load_bonds: every atom (the rows below are read up to n only)
constexpr int MAX_ORDER = 3, MAX_TYPE = 4;

struct Wave {                             // one record's staging area
  unsigned char adj[MA * 32];             // symmetric bond orders over original atom indices, diagonal 0
  unsigned core[32];                      // bit j = atom j is a core neighbour of this core atom; 0 for an atom outside the core
};

__device__ __forceinline__ unsigned low32(unsigned long long ballot) { return (unsigned)ballot; }   // atoms live in lanes 0..28

__global__ __launch_bounds__(64 * DSK_WAVES) void k_scaffold(const unsigned char* __restrict__ rec, const int32_t* __restrict__ n_atoms, int64_t P,
                                                             int32_t* __restrict__ scaffold_mask, int32_t* __restrict__ ring_mask,
                                                             int32_t* __restrict__ summary, unsigned char* __restrict__ status) {
  __shared__ Wave S[DSK_WAVES];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * DSK_WAVES + wave;
  const bool live = p < P;
  const int n = live ? ds_rec::atoms_of(n_atoms, p) : 0;            // a wave without a record passes n = 0 and touches no record
  const unsigned char* __restrict__ mine = rec + (live ? p : 0) * DS_RECORD_BYTES;
  Wave& W = S[wave];
  const bool active = lane < n;
  const unsigned me = lane < 32 ? 1u << lane : 0u;

  int type = 0;
  if (active) type = mine[DS_REC_TYPE + lane];
  bool bad = type > MAX_TYPE;
  if (n > 0) ds_rec::load_bonds(W.adj, mine, ALL, lane);
  __syncthreads();
  unsigned nb = 0u, nb_multiple = 0u;                                // bonded by any order / by order >= 2
  if (active)
    for (int j = 0; j < n; ++j) {
      const unsigned b = W.adj[lane * 32 + j];
      bad |= b > (unsigned)MAX_ORDER;
      nb |= (b ? 1u : 0u) << j;
      nb_multiple |= (b >= 2u ? 1u : 0u) << j;
    }
  const bool usable = n > 0 && __ballot(active && bad) == 0ull;
  const bool on = usable && active;

  // the heavy graph: hydrogens and all their bonds go first
  const unsigned heavy = low32(__ballot(on && type != 0));
  const unsigned hnb = (heavy & me) ? nb & heavy : 0u;

  // the 2-core: a round deletes every atom with at most one neighbour left; at most n rounds kill somebody
  unsigned alive = heavy;
  for (int round = 0; round < n; ++round) {
    const unsigned dead = low32(__ballot((alive & me) && __popc(hnb & alive) <= 1));
    if (!dead) break;
    alive &= ~dead;
  }
  const unsigned core = alive;
  const bool in_core = (core & me) != 0u;
  const unsigned cnb = in_core ? hnb & core : 0u;
  if (lane < 32) W.core[lane] = cnb;
  __syncthreads();

  // exocyclic atoms: one heavy neighbour, it is in the core, the bond to it is multiple
  const bool exo = (heavy & me) && !in_core && __popc(hnb) == 1 && (hnb & core) && (hnb & nb_multiple);
  const unsigned exocyclic = low32(__ballot(exo));

  // ring atoms: a core bond me-b is a ring bond iff me is reached from b without it.  Every atom is expanded at most once per test and a
  // test ends when nothing is left to expand, so a lane runs at most popcount(cnb) * n steps; the first ring bond settles the atom.
  bool ring_atom = false;
  for (unsigned far = cnb; far && !ring_atom; far &= far - 1u) {
    const int b = __ffs((int)far) - 1;
    unsigned reached = 1u << b, todo = (W.core[b] & ~me) & ~reached;   // b expanded here, without its bond to me
    reached |= todo;
    while (todo && !(reached & me)) {
      const int j = __ffs((int)todo) - 1;
      todo &= todo - 1u;
      const unsigned fresh = W.core[j] & ~reached;
      reached |= fresh;
      todo |= fresh & ~me;
    }
    ring_atom = (reached & me) != 0u;
  }
  const unsigned ring_atoms = low32(__ballot(ring_atom));

  // components of the core: comp = the core atoms known to be connected to this one; a round ORs in what they know, so the reach doubles
  unsigned comp = in_core ? (cnb | me) : 0u;
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
  const int components = __popcll(__ballot(in_core && __ffs((int)comp) - 1 == lane));
  int ends = __popc(cnb);                                             // both ends of every core bond
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ends += __shfl_xor(ends, o, 64);
  ends = uniform_i(ends);
  const int rings = ends / 2 - __popc(core) + components;

  if (live) {
    const unsigned scaffold = core | exocyclic;
    if (lane < 4) {
      const int v = lane == 0 ? __popc(heavy) : lane == 1 ? __popc(scaffold) : lane == 2 ? rings : __popc(ring_atoms);
      summary[p * 4 + lane] = usable ? v : 0;
    }
    if (lane == 0) {
      scaffold_mask[p] = (int32_t)(usable ? scaffold : 0u);
      ring_mask[p] = (int32_t)(usable ? ring_atoms : 0u);
      status[p] = (unsigned char)(usable ? DSK_OK : DSK_UNUSABLE);
    }
  }
}

static_assert(DSK_WAVES >= 1 && 64 * DSK_WAVES <= 1024, "a workgroup of whole waves");
static_assert(MA <= 29, "an atom mask fits a 32-bit word with lanes 29..31 clear");

}  // namespace

extern "C" int dsk_scaffold_masks(const uint8_t* rec, const int32_t* n, int64_t P, int32_t* scaffold_mask, int32_t* ring_mask, int32_t* summary,
                                  uint8_t* status, void* stream) {
  const int go = ds_rec::check_table(true, P, rec, n, {scaffold_mask, ring_mask, summary, status});
  if (go != ds_rec::LAUNCH) return go;
  hipLaunchKernelGGL(k_scaffold, dim3((unsigned)((P + DSK_WAVES - 1) / DSK_WAVES)), dim3(64 * DSK_WAVES), 0, (hipStream_t)stream, rec, n, P,
                     scaffold_mask, ring_mask, summary, status);
  return DST_CHECK_LAUNCH();
}
