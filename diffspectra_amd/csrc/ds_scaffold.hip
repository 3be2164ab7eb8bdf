// diffspectra_amd - scaffold analytics on result records: the Bemis-Murcko scaffold atoms (the 2-core of the heavy graph plus its exocyclic
// atoms), the ring atoms and the ring count behind the "Scaf" number of the reference's set metrics.  include/diffspectra_scaffold.h states
// every definition (heavy graph, core, exocyclic atoms, ring bonds, the cyclomatic ring count, the unusable rule); DESIGN.md section 18 has
// the method and the round bound.
//
// One wave64 per record, DSK_WAVES records per workgroup, an atom per lane.  LDS holds, per wave, the bond matrix of ds_rec::load_bonds and one
// word per atom: its neighbours inside the core.  The pruning and the component growth are wave-wide (ballots, shuffles) and run outside
// divergent code; a lane's ring-bond tests read other atoms' words inside divergent loops, so they read LDS and never shuffle.  Integers
// only, no atomics, no early exit: a wave without a record takes part in the workgroup's barriers and writes nothing.  From ds_perceive.h: the
// record scan, reach for the ring test over the core, the component doubling, the wave sum.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/diffspectra_scaffold.h"
#include "ds_perceive.h"
#include "ds_host.h"   // DST_CHECK_LAUNCH

namespace {

using namespace ds_perceive;

struct Wave {                             // one record's staging area
  unsigned char adj[MA * 32];             // symmetric bond orders over original atom indices, diagonal 0
  unsigned core[32];                      // bit j = atom j is a core neighbour of this core atom; 0 for an atom outside the core
};

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
  const unsigned me = lane < 32 ? 1u << lane : 0u;
  const Atom A = scan(W.adj, mine, n, lane, ds_refine::Block{});
  const bool usable = usable_record(A, n), on = usable && A.active;
  const unsigned nb = A.nb, nb_multiple = A.nb2 | A.nb3;             // bonded by any order / by order >= 2

  // the heavy graph: hydrogens and all their bonds go first
  const unsigned heavy = low32(__ballot(on && A.type != H));
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
    const unsigned first = W.core[b] & ~me & ~(1u << b);             // b expanded here, without its bond to me
    ring_atom = (reach(W.core, (1u << b) | first, first, me) & me) != 0u;
  }
  const unsigned ring_atoms = low32(__ballot(ring_atom));

  // components of the core: comp = the core atoms known to be connected to this one; a round ORs in what they know, so the reach doubles
  const unsigned comp = components(in_core ? (cnb | me) : 0u, n);
  const int parts = __popcll(__ballot(in_core && __ffs((int)comp) - 1 == lane));
  const int ends = wave_sum(__popc(cnb));                             // both ends of every core bond
  const int rings = ends / 2 - __popc(core) + parts;

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

}  // namespace

extern "C" int dsk_scaffold_masks(const uint8_t* rec, const int32_t* n, int64_t P, int32_t* scaffold_mask, int32_t* ring_mask, int32_t* summary,
                                  uint8_t* status, void* stream) {
  const int go = ds_rec::check_table(true, P, rec, n, {scaffold_mask, ring_mask, summary, status});
  if (go != ds_rec::LAUNCH) return go;
  hipLaunchKernelGGL(k_scaffold, dim3((unsigned)((P + DSK_WAVES - 1) / DSK_WAVES)), dim3(64 * DSK_WAVES), 0, (hipStream_t)stream, rec, n, P,
                     scaffold_mask, ring_mask, summary, status);
  return DST_CHECK_LAUNCH();
}
