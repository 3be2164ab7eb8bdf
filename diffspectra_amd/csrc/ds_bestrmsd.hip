// diffspectra_amd - symmetry-corrected Kabsch RMSD of the evaluation path: the smallest RMSD after the best rigid fit over ALL graph
// isomorphisms between the generated molecule and its ground truth, for a rotation (proper) and for the mirror image (improper) at once.
// include/diffspectra_rmsd.h states every definition (selection, the trace formula, twins of hydrogen leaves, the verdicts); DESIGN.md
// section 26 has the method, the soundness of the hydrogen-twin rule and the figures.
//
// One wave64 per pair, one wave per workgroup: the generated molecule in lanes 0..28, the ground truth in lanes 32..60, as k_stereo_identity.
// The search is ds_refine.h's, joined here in the order its comment prescribes and going on after every verified leaf, as ds_sites::search
// does; the leaf action is a Kabsch fit: H summed by nine lanes in one fixed order, made wave-uniform through LDS, one fp64 Jacobi SVD
// (ds_svd3.h) in every lane alike.  The best scores and this lane's image under the two best isomorphisms live in registers.  No atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/diffspectra_rmsd.h"
#include "ds_records.h"
#include "ds_refine.h"
#include "ds_sites.h"   // twin_key, count_twins, half_of
#include "ds_svd3.h"
#include "ds_host.h"    // DST_CHECK_LAUNCH

namespace {

using ds_rec::MA;
using ds_sites::half_of;
constexpr unsigned ALL = ~0u;             // keep mask of ds_rec::load_bonds: every atom (the rows are read up to n only)

struct Store {                            // arrays of 64 are indexed by lane
  unsigned char adj[2][MA * 32];
  unsigned key[64];                       // twin key
  unsigned char type[64], fc[64], ord[64];
  unsigned long long sig[64], f[64];      // signatures being ranked; per-atom colour hash of the running round
  unsigned char stack[MA][64];            // the pair search's fields, as ds_refine.h names them
  int cell[MA], atom[MA], cursor[MA];
  unsigned char inv[64], img[32];
  double x[2][32][3];                     // positions of both sides, centred on the centroid of the own selection; 0 for an atom that is not selected
  double h[9];                            // H of the leaf at hand, row-major
  __device__ __forceinline__ const unsigned char* bonds(int side) const { return adj[side]; }
};

__global__ __launch_bounds__(64) void k_best_rmsd(const unsigned char* __restrict__ prb_rec, const int32_t* __restrict__ prb_n,
                                                  const unsigned char* __restrict__ ref_rec, const int32_t* __restrict__ ref_n,
                                                  const int64_t* __restrict__ ref_index, int64_t M, int max_nodes, int all_atoms,
                                                  unsigned char* __restrict__ verdict, double* __restrict__ rmsd, int32_t* __restrict__ count,
                                                  int32_t* __restrict__ nodes, int32_t* __restrict__ found, int32_t* __restrict__ map) {
  __shared__ Store S;
  const int64_t p = blockIdx.x;
  const int lane = threadIdx.x, idx = lane & 31, side = lane >> 5;
  const ds_rec::Pair q = ds_rec::pair_of(p, prb_rec, prb_n, ref_rec, ref_n, ref_index, M);
  const double nan = __builtin_nan("");
  int out = DSR_INVALID, used = 0, isos = 0, selected_a = 0;
  int image0 = -1, image1 = -1;           // this lane's image under the best proper / improper isomorphism
  double value0 = nan, value1 = nan;
  if (q.valid) {
    const int ng = q.n_prb(), nr = q.n_ref();
    const int mine_n = side ? nr : ng;
    const bool active = idx < mine_n;
    const unsigned char* __restrict__ mine = side ? q.ref : q.prb;
    ds_rec::load_bonds(S.adj[0], q.prb, ALL, lane);
    ds_rec::load_bonds(S.adj[1], q.ref, ALL, lane);
    unsigned type = 0u, fc = 0u;
    double px = 0.0, py = 0.0, pz = 0.0;
    if (active) {
      type = mine[DS_REC_TYPE + idx];
      fc = mine[DS_REC_FC + idx];
      const float* __restrict__ xyz = reinterpret_cast<const float*>(mine + DS_REC_POS) + idx * 3;
      px = (double)xyz[0]; py = (double)xyz[1]; pz = (double)xyz[2];
    }
    const bool selected = active && (all_atoms || type != 0u);
    selected_a = (int)__popc(half_of(__ballot(selected), 0));
    out = DSR_DIFFERENT;
    if (ng == nr) {
      const int n = ng;
      __syncthreads();                                         // the bond matrices are in place
      // twins: hydrogen leaves in HEAVY mode only - every other atom keeps its own key and ordinal 0
      const unsigned char* __restrict__ adj = S.adj[side];
      unsigned nbr = 0u;
      if (active)
        for (int j = 0; j < n; ++j) nbr |= (adj[idx * 32 + j] ? 1u : 0u) << j;
      const int parent = __ffs((int)nbr) - 1;
      const bool h_leaf = active && !all_atoms && type == 0u && __popc(nbr) == 1;
      const unsigned key = ds_sites::twin_key(h_leaf ? 1 : 2, parent, h_leaf ? adj[idx * 32 + parent] : 0u, type, fc, lane);
      S.key[lane] = key;
      S.type[lane] = (unsigned char)type;
      S.fc[lane] = (unsigned char)fc;
      S.x[side][idx][0] = selected ? px : 0.0;
      S.x[side][idx][1] = selected ? py : 0.0;
      S.x[side][idx][2] = selected ? pz : 0.0;
      __syncthreads();
      const int ord = active ? ds_sites::count_twins(S.key + side * 32, key, n, idx).ord : 0;
      S.ord[lane] = (unsigned char)ord;
      // centroid of the own side's selection, summed over ascending atom index in every lane alike
      const int mine_sel = (int)__popc(half_of(__ballot(selected), side));
      double cx = 0.0, cy = 0.0, cz = 0.0;
      for (int j = 0; j < n; ++j) { cx += S.x[side][j][0]; cy += S.x[side][j][1]; cz += S.x[side][j][2]; }
      const double inv_sel = mine_sel ? 1.0 / (double)mine_sel : 0.0;
      __syncthreads();                                         // every lane has read the raw positions
      S.x[side][idx][0] = selected ? px - cx * inv_sel : 0.0;
      S.x[side][idx][1] = selected ? py - cy * inv_sel : 0.0;
      S.x[side][idx][2] = selected ? pz - cz * inv_sel : 0.0;
      __syncthreads();
      double G = 0.0;                                          // sum |a_i|^2 + sum |b_i|^2, one order in every lane
      for (int s = 0; s < 2; ++s)
        for (int j = 0; j < n; ++j) G += S.x[s][j][0] * S.x[s][j][0] + S.x[s][j][1] * S.x[s][j][1] + S.x[s][j][2] * S.x[s][j][2];

      // initial colour: (type, charge, ordinal) ranked jointly
      const ds_refine::Ranked first = ds_refine::rank_jointly<true>(S, (unsigned long long)(type << 16 | fc << 8 | (unsigned)ord), n, lane, ds_refine::Block{});
      int colour = active ? first.colour : 0;
      unsigned long long multi = 0ull;
      int st = __ballot(active && first.eq_g != first.eq_r) ? ds_refine::MISMATCH : ds_refine::refine<true>(S, colour, active, n, lane, multi, ds_refine::Block{});
      int depth = 0;                                           // open levels: S.stack[0 .. depth-1]
      bool ended = false;                                      // the search stopped for another reason than the budget
      double best0 = -__builtin_inf(), best1 = -__builtin_inf();   // largest s0 + s1 + d s2 / s0 + s1 - d s2 so far
      int to0 = -1, to1 = -1;
      const auto same_label = [](int a, int b) { return S.type[a] == S.type[b] && S.fc[a] == S.fc[b] && S.ord[a] == S.ord[b]; };
      for (int it = 0; it <= max_nodes; ++it) {                // every pass but the last spends one search node
        if (st == ds_refine::DISCRETE && ds_refine::verify(S, colour, active, n, lane, same_label)) {
          const int to = active && side == 0 ? S.img[idx] : -1;
          ++isos;
          if (lane < 9) {                                      // entry (r, c) of H over ascending generated atom
            const int r = lane / 3, c = lane - 3 * r;
            double h = 0.0;
            for (int i = 0; i < n; ++i) h += S.x[0][i][r] * S.x[1][S.img[i]][c];
            S.h[lane] = h;
          }
          __syncthreads();
          double H[3][3], U[3][3], sv[3], V[3][3];
#pragma unroll
          for (int k = 0; k < 9; ++k) H[k / 3][k % 3] = S.h[k];
          svd3(H, U, sv, V);
          const double det = H[0][0] * (H[1][1] * H[2][2] - H[1][2] * H[2][1]) - H[0][1] * (H[1][0] * H[2][2] - H[1][2] * H[2][0]) +
                             H[0][2] * (H[1][0] * H[2][1] - H[1][1] * H[2][0]);
          const double ds2 = det >= 0.0 ? sv[2] : -sv[2];
          const double e0 = sv[0] + sv[1] + ds2, e1 = sv[0] + sv[1] - ds2;
          if (e0 > best0) { best0 = e0; to0 = to; }            // "greater than": the first isomorphism met wins a tie
          if (e1 > best1) { best1 = e1; to1 = to; }
        }
        if (st == ds_refine::CELLS) {
          if (depth >= MA) break;                              // (cannot happen: every level makes one more generated atom a class of its own)
          ds_refine::open_level(S, depth, colour, active, lane, multi);
        }
        const ds_refine::Try t = ds_refine::next_try(S, depth, colour, active, lane);
        if (t.w < 0) { ended = true; break; }                  // nothing left to try anywhere: every isomorphism has been met
        if (used >= max_nodes) break;                          // the budget does not cover this try: undecided
        ++used;
        st = ds_refine::individualise(S, depth, t, colour, active, n, lane, multi);
      }
      out = !ended ? DSR_UNDECIDED : isos ? DSR_DECIDED : DSR_DIFFERENT;
      if (out == DSR_DECIDED) {
        const double v0 = (G - 2.0 * best0) / (double)selected_a, v1 = (G - 2.0 * best1) / (double)selected_a;
        value0 = sqrt(v0 < 0.0 ? 0.0 : v0);                    // (a NaN stays one: count = 0 is 0 / 0)
        value1 = sqrt(v1 < 0.0 ? 0.0 : v1);
        image0 = to0;
        image1 = to1;
      }
    }
  }
  if (lane < MA) {
    map[(p * 2 + 0) * MA + lane] = image0;
    map[(p * 2 + 1) * MA + lane] = image1;
  }
  if (lane < 2) rmsd[p * 2 + lane] = lane ? value1 : value0;
  if (lane == 0) {
    verdict[p] = (unsigned char)out;
    count[p] = selected_a;
    nodes[p] = used;
    found[p] = isos;
  }
}

static_assert(DSR_DIFFERENT == DS_GRAPH_DIFFERENT && DSR_DECIDED == DS_GRAPH_IDENTICAL && DSR_UNDECIDED == DS_GRAPH_UNDECIDED &&
              DSR_INVALID == DS_GRAPH_INVALID, "the codes 0..3 mean what DS_GRAPH_* mean");

}  // namespace

extern "C" int dsr_best_rmsd_records(const uint8_t* prb_rec, const int32_t* prb_n, int64_t P, const uint8_t* ref_rec, const int32_t* ref_n, int64_t M,
                                     const int64_t* ref_index, int32_t max_nodes, int32_t atoms, uint8_t* verdict, double* rmsd, int32_t* count,
                                     int32_t* nodes, int32_t* found, int32_t* map, void* stream) {
  const bool scalars_ok = max_nodes >= 0 && max_nodes <= DS_GRAPH_MAX_NODES && (atoms == DSR_ATOMS_HEAVY || atoms == DSR_ATOMS_ALL);
  const int go = ds_rec::check_pairs(scalars_ok, P, M, prb_rec, prb_n, ref_rec, ref_n, ref_index, {verdict, rmsd, count, nodes, found, map});
  if (go != ds_rec::LAUNCH) return go;
  hipLaunchKernelGGL(k_best_rmsd, dim3((unsigned)P), dim3(64), 0, (hipStream_t)stream, prb_rec, prb_n, ref_rec, ref_n, ref_index, M,
                     (int)max_nodes, (int)(atoms == DSR_ATOMS_ALL), verdict, rmsd, count, nodes, found, map);
  return DST_CHECK_LAUNCH();
}
