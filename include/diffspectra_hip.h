/*
 * diffspectra_hip.h — C-ABI of the MI355X (gfx950) DMT + SpecFormer denoising library.
 *
 * The reference (AzureLeon1/DiffSpectra) is pure Python: its "FFI" for this path is the Python call
 * convention of SURVEY §8b.  This library is what a binding for that path attaches to: plain device
 * pointers + sizes + a hipStream_t, no torch types, int status returns (0 = ok, <0 = error; the
 * Python mirror turns them into RuntimeError).  All buffers are caller-owned device memory
 * (PyTorch-ROCm allocations in the shipped host code); weights are a caller-owned packed buffer
 * described by ds_weights.  The library's own state is process-global and never changes a result:
 * the stream-mode switch (ds_set_two_stream), the node-row tile switch (ds_set_node_tile, diffspectra_tiles.h), one side stream with its events per device
 * (ds_forward), the compute-unit count per device, and the timing hook (ds_profile_config).
 *
 * Reference interfaces replaced (file:line in /root/reference):
 *   ds_forward            DMT.forward                         models/dmt.py:306-412
 *                         EquivariantMixBlock.forward         models/dmt.py:122-174
 *                         MultiCondEquiUpdate.forward         models/dmt.py:37-60
 *                         TransMixLayer.forward/message       models/layers.py:131-186
 *                         CondGaussianLayer / gaussian        models/layers.py:291-295,328-334
 *                         LearnedSinusodialposEmb + time_mlp  models/layers.py:283-288, dmt.py:249-257,353-357
 *   ds_sampler_step       AncestralSampler.sampling loop body sampling.py:604-624 + models/utils.py:67-106
 *   ds_initial_noise /    sample_combined_position_feature_noise, sample_symmetric_edge_feature_noise
 *   ds_sampler_step_philox                                    models/utils.py:67-106 (+ sampling.py:442-447,604-624)
 *   ds_post_process       post_process + inverse scaler       sampling.py:53-97, utils.py:88-103
 *   ds_check_stability    check_stability (distance half)     evaluation/stability.py:40-73, evaluation/bond_analyze.py:108-133
 *   ds_match_records      hungarian_atom_mapping              eval_sampled_mols/rmsd.py:12-73,106-128,153-227
 *   ds_graph_identity_records   the InChIKey comparison behind Top-K accuracy   compute_metrics.py:222-230, run_lib.py:141
 *   ds_graph_hash_records       the uniqueness count                           evaluation/rdkit_metric.py
 *   ds_mces_records             MCES (Average): one myopic_mces ILP per pair   compute_metrics.py:235-243, run_lib.py:149
 *   ds_morgan_records /         Tanimoto / cosine similarity of radius-2 Morgan fingerprints   compute_metrics.py:246-253
 *   ds_morgan_similarity_records
 *   ds_geometry_count_records / cal_bond_distance, cal_bond_angle, cal_dihedral_angle          evaluation/cal_geometry.py:14-216
 *   ds_geometry_fill_records
 *   ds_mmd_1d_segments          compute_mmd                                                    evaluation/mmd.py:6-63
 *   dsg_group_records /         identify_functional_groups, functional_group_similarity (diffspectra_groups.h)   compute_metrics.py:38-56,117-144
 *   dsg_group_similarity_records
 *   ds_gemm / ds_spec_*   SpecFormer.forward                  models/specformer.py:77-120,167-200,279-309,345-425,457-470
 *
 * Data layout ("packed-ragged", symmetric pair storage — DESIGN.md §3):
 *   node rows   : valid atoms of all molecules, molecule-major           (Nn rows)
 *   pair rows   : unordered pairs a<b of each molecule, upper-triangular row-major,
 *                 p = pair_off[m] + a*(2n-a-1)/2 + (b-a-1)                 (Pp rows)
 *   dense I/O   : xh [B,N,9], edge_x [B,N,N,2] exactly as the reference passes them.
 */
#ifndef DIFFSPECTRA_HIP_H
#define DIFFSPECTRA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DS_OK 0
#define DS_ERR_ARG (-1)
#define DS_ERR_LAUNCH (-2)

#define DS_NBLOCKS 8
#define DS_HID 256
#define DS_EHID 64
#define DS_TDIM 1024
#define DS_ADA_BLOCK_STRIDE 2464 /* 1536 node | 384 edge | 512 equi | 2 dist | pad to 32 */
#define DS_ADA_NODE 0
#define DS_ADA_EDGE 1536
#define DS_ADA_EQUI 1920
#define DS_ADA_DIST 2432
#define DS_ADA_TOP (DS_NBLOCKS * DS_ADA_BLOCK_STRIDE) /* top-level dist_layer scale/shift */
#define DS_ADA_COLS (DS_ADA_TOP + 32)

/* Slots of the packed weight buffer: per-block slots first (DS_W_BLOCK_SLOTS per block), then globals.
 * "W" slots are MFMA-B-operand packed [K/8][2][Npad][4] (k = 8*kg + 4*half + s), zero padded;
 * "B" slots are plain bias vectors padded to Npad. */
enum ds_block_slot {
  DS_BW_EDGE_EMB_W = 0, DS_BW_EDGE_EMB_B,   /* 128 -> 64   rows: [x', rbf63, e64]            dmt.py:139 */
  DS_BW_E0_W, DS_BW_E1_W,                   /* 64 -> 252(256), 64 -> 256, no bias            layers.py:165,183 */
  DS_BW_QKV_W, DS_BW_QKV_B,                 /* 256 -> q252(256)|k252(256)|v256               layers.py:147-149 */
  DS_BW_N2E_W, DS_BW_N2E_B,                 /* 256 -> 64                                      dmt.py:157 */
  DS_BW_FF1_W, DS_BW_FF1_B, DS_BW_FF2_W, DS_BW_FF2_B,   /* 256->512->256                      dmt.py:114-116 */
  DS_BW_FF3_W, DS_BW_FF3_B, DS_BW_FF4_W, DS_BW_FF4_B,   /* 64->128->64                        dmt.py:118-120 */
  DS_BW_NODE_RO_W, DS_BW_NODE_RO_B,         /* 256 -> 64   node_i                            dmt.py:387 */
  DS_BW_EDGE_RO_W, DS_BW_EDGE_RO_B,         /* 64 -> 16(32) edge_i                           dmt.py:388 */
  DS_BW_AC_W,                               /* 256 -> 512  input_lin[:, 0:256] | [:, 256:512] dmt.py:39,45 */
  DS_BW_ED_W, DS_BW_ED_B,                   /* 128 -> 256  input_lin[:, 512:640] rows [e64, dist64] + bias */
  DS_BW_CM0_W, DS_BW_CM0_B,                 /* 256 -> 256  coord_mlp.0                        dmt.py:32 */
  DS_BW_CM2_W,                              /* 256 -> 3(32) coord_mlp.2 (no bias)             dmt.py:34 */
  DS_BW_RBF_MEAN, DS_BW_RBF_STD, DS_BW_RBF_ASTD, /* 63(64): mean, |std|+1e-5, a*std           layers.py:332-334 */
  DS_BW_COORD_SCALE,                        /* 1(32)       CoorsNorm.scale                    layers.py:347 */
  DS_BW_CM0_H,                              /* coord_mlp.0 as two fp16 planes (w = w1 + w2/2048) in f16-MFMA A-operand order:
                                               halves [plane 2][k/16 16][k-half 2][feature 256][8]; see k_equi_pairs */
  DS_BW_E0_H, DS_BW_E1_H,                   /* lin_edge0 / lin_edge1 (64 -> 256) TIMES 2 log2(e) in the same split-fp16 layout: k_attn_fused evaluates
                                               tanh(x) as 1 - 2 / (1 + exp2(2 log2(e) x)) and the factor rides in the weights (engine.TANH_PRESCALE) */
  DS_BW_ED_H,                               /* input_lin edge|dist part (128 -> 256) split-fp16 (k_edge_update) */
  DS_BW_QKV_H,                              /* q|k|v projection (256 -> 768) split-fp16 (k_node_qkv) */
  DS_BW_FF3_H,                              /* ff_linear3 (64 -> 128) split-fp16 (k_edge_update, transposed) */
  DS_BW_FF4_C,                              /* ff_linear4 (128 -> 64) split-fp16 in accumulator-chain order: halves [plane 2][hc 4][s 2][ft 2][lane 64][8],
                                               element j of lane (r, h) = W[ft*32 + r][hc*32 + 16 s + 8 (j>>2) + 4 h + (j&3)] */
  DS_BW_N2E_H, DS_BW_FF1_H, DS_BW_FF2_H, DS_BW_NODE_RO_H, DS_BW_AC_H,   /* the five GEMMs of k_node_update, split-fp16 */
  DS_BW_EDGE_EMB_H,                         /* edge_emb (128 -> 64, rows [x', rbf63, e64]) split-fp16 (k_edge_geom) */
  DS_W_BLOCK_SLOTS
};
enum ds_global_slot {
  DS_GW_SIN_W = 0,                          /* 8(32)       time_mlp.0.weights                 layers.py:285 */
  DS_GW_TM1_W, DS_GW_TM1_B,                 /* 17(24) -> 1024                                 dmt.py:254 */
  DS_GW_TM3_W, DS_GW_TM3_B,                 /* 1024 -> 1024                                   dmt.py:256 */
  DS_GW_ADA_W, DS_GW_ADA_B,                 /* 1024 -> DS_ADA_COLS, all *time_mlp Linears (dmt.py:23-26,102-109; layers.py:321-324);
                                               the weight in the split-fp16 layout of DS_BW_CM0_H: halves [2][64][2][DS_ADA_COLS][8] */
  DS_GW_NODE_EMB_W, DS_GW_NODE_EMB_B,       /* 12(16) -> 256                                  dmt.py:376 */
  DS_GW_EDGE_EMB_W, DS_GW_EDGE_EMB_B,       /* 68(72) -> 64  rows [edge_x2, cond_edge_x2, dist64]  dmt.py:373,377 */
  DS_GW_RBF_MEAN, DS_GW_RBF_STD, DS_GW_RBF_ASTD,
  DS_GW_NP0_W, DS_GW_NP0_B, DS_GW_NP2_W, DS_GW_NP2_B, DS_GW_NP4_W, DS_GW_NP4_B, /* 768->256->128->6(32) dmt.py:227-233 */
  DS_GW_EX0_W, DS_GW_EX0_B, DS_GW_EX2_W, DS_GW_EX2_B, DS_GW_EX4_W, DS_GW_EX4_B, /* edge_exist_mlp 192->64->32->1(32) */
  DS_GW_ET0_W, DS_GW_ET0_B, DS_GW_ET2_W, DS_GW_ET2_B, DS_GW_ET4_W, DS_GW_ET4_B, /* edge_type_mlp  192->64->32->1(32) */
  DS_GW_NP0_H, DS_GW_NP2_H,                 /* node_pred_mlp.0 (768 -> 256) and .2 (256 -> 128) in the split-fp16 layout (k_node_readout) */
  DS_GW_EX0_H, DS_GW_ET0_H,                 /* edge_exist_mlp.0 / edge_type_mlp.0 (192 -> 64) split-fp16 (k_edge_readout) */
  DS_GW_EX2_C, DS_GW_ET2_C,                 /* edge_exist_mlp.2 / edge_type_mlp.2 (64 -> 32) split-fp16 in the accumulator-chain order of DS_BW_FF4_C:
                                               halves [plane 2][hc 2][s 2][ft 1][lane 64][8] (k_edge_readout) */
  DS_W_GLOBAL_SLOTS
};
#define DS_W_NUM_SLOTS (DS_NBLOCKS * DS_W_BLOCK_SLOTS + DS_W_GLOBAL_SLOTS)

#define DS_MAX_ATOMS 29               /* QM9 (data.max_node, configs/diffspectra_qm9s.py:28) */
#define DS_RECORD_BYTES 1248          /* one result record (shard.pack_records_u8): 29*3 f32 positions | 29 u8 types | 29 i8 charges | 29*29 u8 bond orders | pad */
#define DS_REC_POS 0                                              /* byte offsets of a record's fields; DS_REC_BOND_END is where the pad starts */
#define DS_REC_TYPE (DS_MAX_ATOMS * 12)
#define DS_REC_FC (DS_REC_TYPE + DS_MAX_ATOMS)
#define DS_REC_BOND (DS_REC_FC + DS_MAX_ATOMS)
#define DS_REC_BOND_END (DS_REC_BOND + DS_MAX_ATOMS * DS_MAX_ATOMS)
#ifdef __cplusplus
static_assert(DS_REC_BOND_END <= DS_RECORD_BYTES && DS_RECORD_BYTES % 4 == 0, "a record holds its fields and is a whole number of dwords");
static_assert((DS_REC_BOND_END + 3) / 4 * 4 <= DS_RECORD_BYTES, "the dwords that cover the bond block stay inside the record");
#endif

/* Record pairs: the contract that ds_match_records, ds_graph_identity_records, ds_mces_records and ds_morgan_similarity_records share
 * (ds_graph_hash_records and ds_morgan_records take the single-table part of it: one record table, n, alignment, P).
 *   Records   prb_rec [P] / ref_rec [M]: DS_RECORD_BYTES bytes each, fields at the DS_REC_* offsets above - fp32 positions [29][3], atom type
 *             bytes in decoder order H, C, N, O, F, formal-charge bytes (i8), the bond-order matrix [29][29] u8, pad.  Both tables must be
 *             4-byte aligned (records are read as dwords and hold fp32 positions).
 *   Counts    prb_n [P], ref_n [M]: atoms of every molecule, clamped to 0..29.
 *   Bonds     of an unordered atom pair i < j the byte at row i, column j decides (the upper triangle); the diagonal is no pair.
 *   Pairing   pair p compares prb_rec[p] with ref_rec[ref_index[p]], or with ref_rec[p] when ref_index is NULL (identity pairing, which needs
 *             M >= P).  A row outside [0, M) makes the pair INVALID: neither record is read, and every output of the pair has its stated
 *             invalid value.  M = 0 with a ref_index is therefore allowed (ref_rec / ref_n may then be NULL).
 *   P = 0     launches nothing and returns DS_OK, whatever the pointers.
 *   DS_ERR_ARG  checked in this order: the entry point's own scalars (each section names them) together with P < 0, M < 0, P > 2^31 - 1;
 *             then, for P > 0: a NULL prb_rec, prb_n or output; with M > 0 a NULL ref_rec or ref_n; a NULL ref_index with M < P; a table
 *             that is not 4-byte aligned.
 *   One wave per pair, no atomics: a pair's outputs do not depend on the batch. */

typedef struct ds_weights {
  const float* base;                 /* device: packed weights */
  const int64_t* off_dev;            /* device copy of off[] (read by the kernels) */
  int64_t off[DS_W_NUM_SLOTS];       /* float offsets of each slot into base (host copy) */
  float edge_th;                     /* model.edge_quan_th   (dmt.py:192) */
  float spatial_cut_off;             /* model.spatial_cut_off, compared with SQUARED distance (models/utils.py:118-126) */
} ds_weights;

typedef struct ds_layout {
  int32_t B, N, Nn, Pp;              /* molecules, padded atoms per molecule, packed node rows, packed pair rows */
  int32_t max_n;                     /* largest molecule (<= DS_MAX_ATOMS) */
  int32_t _pad;
  const int32_t* node_off;           /* [B+1] packed-node prefix */
  const int32_t* pair_off;           /* [B+1] packed-pair prefix */
  const int32_t* node_dense;         /* [Nn]  dense row b*N+i of packed node */
  const int32_t* node_mol;           /* [Nn]  molecule of packed node */
  const int32_t* pair_a;             /* [Pp]  packed node row of the smaller local index */
  const int32_t* pair_b;             /* [Pp]  packed node row of the larger local index */
  const int32_t* pair_mol;           /* [Pp] */
  const int32_t* mol_by_size;        /* [B][4] {node_off, n, pair_off, n(n-1)/2} of the molecules by descending size: workgroup i of a per-molecule
                                        kernel takes record i - one 16-byte load instead of a chain of dependent ones, and the tail of a launch is
                                        made of the small molecules (NULL: index order through node_off / pair_off) */
} ds_layout;

typedef struct ds_workspace {        /* all device fp32 unless noted; sizes in floats */
  float* pos;        /* [Nn,4]  xyz + pad */
  float* h;          /* [Nn,256] */
  float* e;          /* [Pp,64] */
  float* atom_hids;  /* [Nn,768] */
  float* edge_hids;  /* [Pp,192] */
  float* tfeat;      /* [B,24]   sinusoid features (17 used) */
  float* tmid;       /* [B,1024] */
  float* temb_silu;  /* [B,1024 floats]: SiLU(time_mlp(noise_level) + ctx) as two fp16 planes per row, halves [B][2][1024] (a = a1 + a2/2048) */
  float* ada;        /* [B,DS_ADA_COLS] */
  float* qkv;        /* [Nn,768] */
  float* ye;         /* [Pp,64 floats]: LayerNorm'd + modulated edge features of the current block (dmt.py:149) as two fp16 planes per
                        row, halves [Pp][2][64] (a = a1 + a2/2048): the MFMA operand from which k_attn_fused recomputes
                        tanh(lin_edge0 e) / tanh(lin_edge1 e) per molecule instead of streaming them through HBM */
  float* dist;       /* [Pp]     modulated squared distance x' of the current block (layers.py:330-331); its 64 CondGaussian
                        features are recomputed where they are consumed (k_edge_geom, k_edge_update) */
  float* attn;       /* [Nn,256] */
  float* u;          /* [Nn,64]  node2edge_lin weight applied per node (no bias) */
  float* ac;         /* [Nn,512] input_lin row part | col part */
  float* ed;         /* [Pp,256] input_lin edge+dist part + bias */
  float* lg;         /* [Pp,2,16] attention logits: [p][0] source a -> target b, [p][1] source b -> target a */
  float* tr;         /* [Pp,2,4] per-edge translation vectors of the current block: [p][0] a -> b, [p][1] b -> a */
  int32_t* adj;      /* [Pp]     bit0: cond_adj_2d, bit1: cond_adj_spatial */
  int32_t* flags;    /* [64]     0: any nonzero cond distance, 1: NaN in positions; [16..] diagnostic-build counters */
} ds_workspace;

/* sizeof() of ds_weights, ds_layout, ds_workspace, ds_gemm_args for the binding's layout self-check: out[0..3]. */
void ds_struct_sizes(int64_t* out);

/* Generic fp32-MFMA GEMM: C[M, N] = epilogue(A[M,K] * W + bias).  Wp packed as above with Kpad=ceil8(K),
 * Npad=ceil32(N).  act: 0 none, 1 SiLU, 2 GELU(erf), 3 tanh.  Optional: residual R added after act; per-column
 * affine (col_scale/col_shift, eval-mode BatchNorm) applied last; a_silu!=0 applies SiLU to A on load.
 * Row groups (grp_rows > 0): row r lives at (r / grp_rows) * grp_stride + (r % grp_rows) * ld — used for the
 * unfold view of spectra (specformer.py:105), token-buffer slices (:194) and positional tables (:183-188),
 * for which R row = r % r_grp_rows. */
typedef struct ds_gemm_args {
  const float* A; int64_t lda; int32_t a_grp_rows; int32_t _p0; int64_t a_grp_stride;
  const float* Wp; const float* bias;
  float* C; int64_t ldc; int32_t c_grp_rows; int32_t _p1; int64_t c_grp_stride;
  int32_t M, K, N, act;
  const float* R; int64_t ldr; int32_t r_grp_rows; int32_t a_silu;
  const float* col_scale; const float* col_shift;
} ds_gemm_args;
int ds_gemm(const ds_gemm_args* args, void* stream);

/* The split-fp16 GEMM that the block kernels are built from, as a stand-alone entry point (the per-step adaLN table GEMM uses
 * it; tests measure its accuracy against fp64 through it): C[M, N] = A * W + bias with fp32-level accuracy on the f16 matrix pipe.
 * Every operand value a travels as two fp16 numbers, a = a1 + a2/2048 (a1 = fp16(a) round-to-nearest, a2 = fp16((a - a1)*2048)),
 * the product is a1 b1 + (a1 b2 + a2 b1)/2048: three v_mfma_f32_32x32x16_f16 per 16-deep k-block, fp32 accumulate.
 *   A_split : device, halves [M][2][K] (plane 0 | plane 1 per row), K % 64 == 0
 *   W_split : device, the layout of engine.pack_linear_f16_split: halves [2][K/16][2][N][8], N % 32 == 0, as float* */
int ds_gemm_split(const void* A_split, const float* W_split, const float* bias, float* C, int64_t ldc, int32_t M, int32_t K,
                  int32_t N, void* stream);

/* One DMT evaluation (dmt.py:306-412).  xh [B,N,9], edge_x [B,N,N,2] dense; cond_x/cond_edge_x may be NULL
 * (first step, dmt.py:332-335); noise_level [B]; ctx_emb [B,1024] = cond_lin(SpecFormer(context)) (dmt.py:348-350),
 * NULL means zero context embedding.  out_xh [B,N,9], out_edge [B,N,N,2] are fully written (masked entries 0).
 * The side stream of the two-stream mode (ds_set_two_stream) and its events exist once per device, whatever `stream` is: any number of
 * host threads may run ds_forward on different devices, two must not run it on the same device at the same time. */
int ds_forward(const ds_weights* w, const ds_layout* L, ds_workspace* ws,
               const float* xh, const float* edge_x, const float* cond_x, const float* cond_edge_x,
               const float* noise_level, const float* ctx_emb,
               float* out_xh, float* out_edge, void* stream);

/* ds_forward runs a block's node rows behind the attention (k_node_update) and the next block's q|k|v projection on a library-owned
 * side stream beside the pair rows' k_edge_update (fork / join by events; safe under stream capture).  on = 0: one stream (the order of
 * ds_stage_block), 1: two streams, -1: follow the environment variable DIFFSPECTRA_TWO_STREAM if set, else two streams for small
 * batches only (below ~2 500 molecules: there the side kernels fill launch tails; at the bench size they do not pay).  Returns the previous
 * setting.  Results are bit-identical in both modes.  (Build extension: the reference has no such switch.) */
int ds_set_two_stream(int on);

/* Stage-level entry points (used by the parity tests to localise a mismatch; same kernels ds_forward launches). */
int ds_stage_time(const ds_weights* w, const ds_layout* L, ds_workspace* ws, const float* noise_level,
                  const float* ctx_emb, void* stream);
int ds_stage_init(const ds_weights* w, const ds_layout* L, ds_workspace* ws, const float* xh, const float* edge_x,
                  const float* cond_x, const float* cond_edge_x, void* stream);
int ds_stage_block(const ds_weights* w, const ds_layout* L, ds_workspace* ws, int block, int last, void* stream);
int ds_stage_readout(const ds_weights* w, const ds_layout* L, ds_workspace* ws, float* out_xh, float* out_edge,
                     void* stream);

/* Ancestral update (sampling.py:604-624): x <- c_x*x + c_pred*pred + (sigma*noise)*temperature with the reference's noise
 * transforms fused (mask, CoM projection of position noise, tril(-1)+transpose edge noise: models/utils.py:67-106).
 * raw_pos [B,N,3], raw_feat [B,N,6], raw_edge [B,2,N,N] are the three randn draws.  x_mean/edge_mean receive the
 * noise-free posterior means (what sampling() returns after the last step). */
int ds_sampler_step(const ds_layout* L, float c_x, float c_pred, float sigma, float temperature,
                    float* x, float* edge_x, const float* pred, const float* edge_pred,
                    const float* raw_pos, const float* raw_feat, const float* raw_edge,
                    float* x_mean, float* edge_mean, void* stream);

/* The same two operations with the noise generated IN the kernel: counter-based Philox4x32-10 + Box-Muller, one stream per
 * molecule keyed on (seed, mol_id[m]) and indexed by (draw, atom / unordered atom pair) - never by the molecule's position
 * in the batch, the batch's padded width or the rank that owns it.  A sampling run therefore produces the same molecules
 * however it is cut into micro-batches and ranks, and the three randn launches + raw-noise tensors of the
 * reference's draw order disappear from the step.  Same distributions as models/utils.py:67-106: masked N(0,1), position
 * noise CoM-projected per molecule, edge noise one draw per unordered pair and channel written to both (i,j) and (j,i).
 *   draw 0           : ds_initial_noise  (z_T, edge_z_T of sampling.py:442-447)
 *   draw 1 + step    : ds_sampler_step_philox for denoise step `step` (sampling.py:611-612,623-624)
 * Philox counter = (element, draw, mol_id, kind) with kind 0: atom a, word block j -> element 3a + j (12 normals per atom,
 * 9 used: xyz, 5 type channels, charge); kind 1: pair lo < hi -> element hi(hi-1)/2 + lo (4 normals, 2 used).  Key = seed.
 * mol_id: device int64 [B].  x [B,N,9] / edge_x [B,N,N,2] are fully written by ds_initial_noise (masked entries 0). */
int ds_initial_noise(const ds_layout* L, uint64_t seed, const int64_t* mol_id, float* x, float* edge_x, void* stream);
int ds_sampler_step_philox(const ds_layout* L, float c_x, float c_pred, float sigma, float temperature,
                           uint64_t seed, int32_t step, const int64_t* mol_id,
                           float* x, float* edge_x, const float* pred, const float* edge_pred,
                           float* x_mean, float* edge_mean, void* stream);

/* Graph-replayable form of one denoise iteration: everything that changes from one iteration to the next
 * is read from device memory, so the launch sequence [ds_step_begin, ds_forward, ds_sampler_step_philox_dev] has constant
 * arguments and can be captured once (hipGraph) and replayed - small batches are otherwise bound by host launch work.
 *   table [S,4] device: (c_x, c_pred, sigma, noise_level) per step (sampling.py:572-584,604-606);
 *   step  device int32: ds_step_begin increments it (so it must hold i-1 before iteration i) and fills noise_level[0..B)
 *         with table[*step][3]; ds_sampler_step_philox_dev reads the coefficients and the Philox draw index from *step. */
int ds_step_begin(const float* table, int32_t n_steps, int32_t* step, int32_t B, float* noise_level, void* stream);
int ds_sampler_step_philox_dev(const ds_layout* L, const float* table, const int32_t* step, float temperature,
                               uint64_t seed, const int64_t* mol_id, float* x, float* edge_x, const float* pred,
                               const float* edge_pred, float* x_mean, float* edge_mean, void* stream);

/* post_process (sampling.py:53-97, compress_edge=True, centered=True, normalize_factors 1,4,4,1):
 * pos_out [B,N,3] f32, atom_type [B,N] i32 (argmax), fc [B,N] i32 (round(4*x)), edge_type [B,N,N] f32 in {0,1,2,3}. */
int ds_post_process(const ds_layout* L, const float* xh, const float* edge_x,
                    float* pos_out, int32_t* atom_type, int32_t* fc, float* edge_type, void* stream);

/* 3-D stability check of generated molecules (evaluation/stability.py:40-73 with evaluation/bond_analyze.py:5-45,85,90,
 * 108-133; QM9 atom set H, C, N, O, F): bond order of every atom pair from its distance in picometres (single if
 * 100 d < L1 + 10, then double if a double-bond length exists and 100 d < L2 + 5, then triple if 100 d < L3 + 3), valence
 * of every atom against allowed_bonds.  pos [B,N,3] Angstrom, atom_type [B,N] in 0..4 (the argmax ds_post_process wrote).
 * bond_order [B,N,N] i32 (may be NULL), nr_stable [B] = atoms with the right valence, mol_stable [B] = 1 if all are. */
int ds_check_stability(const ds_layout* L, const float* pos, const int32_t* atom_type, int32_t* bond_order,
                       int32_t* nr_stable, int32_t* mol_stable, void* stream);

/* Structure metric of (generated, ground-truth) molecule pairs, one wave per pair, fp64 (eval_sampled_mols/rmsd.py:12-73,106-128,153-227
 * without RDKit).  Records, counts, bonds, pairing and the argument check are those of "record pairs" above; NaN max_distance is DS_ERR_ARG.
 *   1. each side keeps its largest connected fragment (a bond is an order > 0, read from the upper triangle of the record's bond matrix;
 *      among equally large fragments the one that holds the lowest atom index - RDKit's fragment order under Python's max; fragment atoms
 *      stay in ascending original order) and is centred on that fragment's centroid; a non-finite coordinate in either fragment makes
 *      the pair invalid (the reference's assignment refuses such a cost matrix, rmsd.py:164-168);
 *   2. cost[p][r] = |x_p - x_r| + penalty (0 same type, 2 both in {C, N, O}, 10 otherwise), rows generated, columns ground-truth atoms;
 *   3. minimum-cost assignment of the centred coordinates, unclipped; fewer than min_atoms assigned -> the pair is invalid
 *      (the reference's PCA fallback cannot make such a pair valid and is not built);
 *   4. Kabsch: H = P^T Q over the assigned rows (ascending generated index) = U S V^T, R = U V^T, with the last row of V^T negated when
 *      det R < 0; aligned = centred_generated . R;
 *   5. second assignment on the aligned coordinates with cost entries above max_distance (inf allowed: no clipping) set to 1000; matches
 *      whose clipped cost is <= max_distance are kept; fewer than min_atoms (or none) kept -> invalid.
 * Outputs per pair p:
 *   rmsd      f64  sqrt(mean |aligned_p - centred_r|^2) over the kept map (spatial distance only); NaN if invalid
 *   n_matched i32  size of the kept map whenever step 5 was reached (0 otherwise), also for an invalid pair
 *   type_acc  f32  share of kept matches with equal atom type; 0 if invalid
 *   bond_acc  f32  share of the unordered pairs of mapped generated atoms whose bond order equals that of their images; 0 if invalid
 *   exact     u8   1 when both fragments are the whole molecules, the atom counts agree, every atom is mapped and every type, formal
 *                  charge and bond order agrees under the map: the map is then an explicit graph isomorphism (a certified hit; 0 proves
 *                  nothing - a correct graph in another conformation can miss - so hit@K from it is a LOWER bound)
 *   map [P,29] i32 ground-truth atom of every generated atom (original indices), -1 where unmatched / invalid
 * (bond_acc / exact are build extensions.) */
int ds_match_records(const uint8_t* prb_rec, const int32_t* prb_n, int64_t P, const uint8_t* ref_rec, const int32_t* ref_n, int64_t M,
                     const int64_t* ref_index, float max_distance, int32_t min_atoms, double* rmsd, int32_t* n_matched,
                     float* type_acc, float* bond_acc, uint8_t* exact, int32_t* map, void* stream);

/* Molecular-graph identity of (generated, ground-truth) pairs, one wave per pair, integers only: is there a bijection of the atoms that
 * preserves the decoder atom type, the formal-charge byte and the bond-order byte of every atom pair?  Records, counts, bonds, pairing and the
 * argument check are those of "record pairs" above; coordinates are
 * never read, so the answer does not depend on the conformation.  Whole molecules are compared, disconnected pieces included; unequal atom
 * counts are different; two 0-atom molecules are identical with an empty map.
 *   This is identity of the CONSTITUTION.  It is not InChIKey identity, which the reference compares (compute_metrics.py:222-230): there is
 *   no stereo layer (enantiomers and E/Z isomers are identical here) and no InChI normalisation (two tautomers, or two ways of writing a
 *   charge-separated group, are different here; dsm_normal_records of diffspectra_mobile.h rewrites a record so that they are not).
 * Method: individualisation-refinement.  Colour = joint rank of (type, charge) over both molecules; a refinement round ranks, again jointly,
 * (own colour, multiset of (bond order, neighbour colour) over the bonded neighbours) until the number of classes stops growing.  Differing
 * colour histograms prove the graphs different; all classes singletons leaves one candidate bijection, which is verified byte by byte;
 * otherwise the lowest generated atom of the lowest class with several atoms is individualised against every ground-truth atom of that
 * class in ascending order (one SEARCH NODE per try), depth first, the first verified bijection wins.
 *   verdict u8  DS_GRAPH_IDENTICAL  map is an isomorphism that the kernel has checked explicitly (every type, charge and bond byte)
 *               DS_GRAPH_DIFFERENT  proven: unequal atom counts, an invariant mismatch at the root, or an exhausted search
 *               DS_GRAPH_UNDECIDED  a further try would exceed max_nodes (max_nodes = 0 is plain colour refinement)
 *               DS_GRAPH_INVALID    ref_index outside [0, M): nothing is read
 *   nodes  i32  search nodes used (0 when refinement alone decides)
 *   map [P,29] i32  ground-truth atom of every generated atom when verdict = DS_GRAPH_IDENTICAL, -1 everywhere otherwise
 * max_nodes outside [0, DS_GRAPH_MAX_NODES] is DS_ERR_ARG.  Every loop of the kernel is bounded (rounds <= n + 1, depth <= n, tries <=
 * max_nodes): a malformed record ends in a verdict. */
#define DS_GRAPH_DIFFERENT 0
#define DS_GRAPH_IDENTICAL 1
#define DS_GRAPH_UNDECIDED 2
#define DS_GRAPH_INVALID 3
#define DS_GRAPH_MAX_NODES 1048576    /* 1 << 20 */
int ds_graph_identity_records(const uint8_t* prb_rec, const int32_t* prb_n, int64_t P, const uint8_t* ref_rec, const int32_t* ref_n, int64_t M,
                              const int64_t* ref_index, int32_t max_nodes, uint8_t* verdict, int32_t* nodes, int32_t* map, void* stream);

/* Permutation-invariant 64-bit hash of the labelled graph of every record, one wave per molecule (record table, counts, bonds, alignment and P as in
 * "record pairs" above).
 * All arithmetic is unsigned 64-bit with wrap-around.  With
 *   fmix(x):    x ^= x >> 30;  x *= 0xbf58476d1ce4e5b9;  x ^= x >> 27;  x *= 0x94d049bb133111eb;  x ^= x >> 31
 *   mix(a, b) = fmix(a + 0x9e3779b97f4a7c15 * (b + 1))
 * the atoms start at h_i = mix(type_i, charge_i) (both as the unsigned byte of the record), then 29 rounds of
 *   h_i <- mix(h_i, sum over j != i with bond_ij > 0 of mix(h_j, bond_ij))          (all h_j of the previous round)
 * and hash = mix(n, sum_i fmix(h_i)).  Identical graphs have equal hashes by construction.  Equal hashes do NOT prove identity: molecules
 * that colour refinement cannot tell apart (a hexagon and two triangles of one atom type) collide on purpose, and 64 bits can collide
 * by chance; ds_graph_identity_records decides. */
int ds_graph_hash_records(const uint8_t* rec, const int32_t* n, int64_t P, uint64_t* hash, void* stream);

/* Exact MCES (maximum common edge subgraph) distance of (generated, ground-truth) pairs, one wave per pair, integers only: how far a wrong
 * molecule is from the right one as a labelled graph.  Replaces the reference's "MCES (Average)" (compute_metrics.py:235-243, run_lib.py:149:
 * one myopic_mces ILP per pair through pulp, on SMILES made by RDKit).  Records, counts, bonds, pairing and the argument check are those of
 * "record pairs" above; coordinates are never read.  drop_h = 1 leaves out the atoms of decoder type 0
 * (hydrogen) and their bonds, as the reference's SMILES route does; drop_h = 0 keeps every atom.
 *   A bond's weight w is its bond-order byte, an integer.  The formal-charge byte is NOT compared (myopic_mces labels nodes by element only).
 *   A common subgraph is a partial injective map pi from atoms of A (generated) to atoms of B (ground truth) of the same type.
 *     score(pi) = sum over bonds (i, j) of A with both ends mapped and (pi i, pi j) bonded in B of min(w_A(i, j), w_B(pi i, pi j))
 *     dist      = W_A + W_B - 2 max_pi score(pi),   W = a side's total bond weight
 *   which restates the myopic_mces objective: an unmatched bond costs its weight, a matched one |w - w'|.  dist is an integer, symmetric in A
 *   and B, and 0 exactly when the kept graphs, their bondless atoms set aside (an atom without a bond has no edge to lose: methane / water is
 *   0), are identical up to the formal charges.
 * Two deviations from the reference's number:
 *   - the records hold Kekule orders 1..3, not RDKit's aromatic 1.5, so two Kekule drawings of one substituted ring are a non-zero distance
 *     apart (o-xylene, its two drawings: 2; benzene: 0);
 *   - parity with the myopic_mces package itself is unpinned: it cannot be run where this project runs.  The tests compare with the same
 *     integer program restated on scipy.optimize.milp and with exhaustive enumeration (tests/mces_mirror.py).
 * Method: depth-first branch-and-bound.  The atoms of A are ordered (largest weighted degree first, then the largest bond weight into the
 * atoms already ordered, ties to the larger weighted degree, then the lower index); at a level every unused ground-truth atom of the same
 * type is a candidate image, tried in descending gain (score added by the bonds into already-mapped neighbours; lowest index on ties), then
 * "unmapped".  One try is one SEARCH NODE.  A try whose score beats the best so far becomes the best map at once (a partial map is a common
 * subgraph).  The search descends only if bound > best, bound = score + min(rem_a, rem_b):
 *     ub_A(e) = max over bonds f of B whose end types match e's of min(w_e, w_f); ub_B likewise
 *     rem_a   = sum of ub_A(e) over bonds of A with an undecided end and no end decided "unmapped"
 *     rem_b   = sum of ub_B(f) over bonds of B whose ends are not both used
 * and the remaining images of a level are skipped once score + gain + rem_a <= best.  The search ends when best reaches the root bound
 * min(sum ub_A, sum ub_B) or nothing is left to try.
 * Soundness: every bond of A that can still add to the score has an undecided end and no end left out, and adds at most ub_A; a bond of B
 * with both ends used has its preimage decided, so its share is in the score, and every other adds at most ub_B once - both terms are upper
 * bounds on any completion, so a skipped subtree holds nothing better than best.  dist is computed from a map the kernel holds (returned in
 * `map`), so it is an upper bound whatever the budget; lower comes from the root bound.  (Types beyond the seventh distinct one of a pair
 * share one class in ub only, which can only raise the bound.)
 *   dist   i32  W_A + W_B - 2 best: an upper bound that `map` achieves; the distance when status = DS_MCES_EXACT
 *   lower  i32  W_A + W_B - 2 (root bound) when undecided, = dist when exact
 *   status u8   DS_MCES_EXACT      the search was exhausted or best reached the root bound
 *               DS_MCES_UNDECIDED  a further try would exceed max_nodes: lower <= distance <= dist
 *               DS_MCES_INVALID    ref_index outside [0, M): nothing is read, dist = lower = -1, map all -1
 *   nodes  i32  tries used
 *   map [P,29] i32  ground-truth atom of every generated atom in the best map (original indices), -1 where unmapped or dropped
 * max_nodes outside [0, DS_MCES_MAX_NODES] and drop_h outside {0, 1} are DS_ERR_ARG.  Every loop of the kernel is bounded (depth <= 29,
 * passes <= 2 max_nodes + 64): a malformed record ends in a verdict. */
#define DS_MCES_EXACT 0
#define DS_MCES_UNDECIDED 2
#define DS_MCES_INVALID 3
#define DS_MCES_MAX_NODES 4194304     /* 1 << 22 */
int ds_mces_records(const uint8_t* prb_rec, const int32_t* prb_n, int64_t P, const uint8_t* ref_rec, const int32_t* ref_n, int64_t M,
                    const int64_t* ref_index, int32_t drop_h, int32_t max_nodes, int32_t* dist, int32_t* lower, uint8_t* status,
                    int32_t* nodes, int32_t* map, void* stream);

/* Morgan (ECFP-like) fingerprints of the labelled graph of every record, and the sizes from which the Tanimoto and the cosine similarity of
 * the fingerprints of (generated, ground-truth) pairs follow - the reference's "Tanimoto (Morgan)" and "Cosine (Morgan)"
 * (compute_metrics.py:246-253: GetMorganFingerprintAsBitVect(mol, 2, nBits=2048), TanimotoSimilarity, CosineSimilarity) without RDKit.  One
 * wave per molecule / per pair, integers only.  All arithmetic is unsigned 64-bit with wrap-around; fmix and mix(a, b) are those of
 * ds_graph_hash_records above.  Records, counts, bonds, pairing and the argument check are those of "record pairs" above; coordinates are
 * never read.
 *   Kept atoms   the atoms i < n (n clamped to 0..29); with drop_h = 1 only those whose type byte is not 0.
 *   Kept bonds   the unordered pairs of kept atoms whose bond byte (upper triangle) is > 0; the bond order is that byte.
 *   Atom invariant of a kept atom i:
 *     d_i  the number of kept bonded neighbours;
 *     h_i  the number of bonded neighbours of type 0 when drop_h = 1, else 0;
 *     c_i  1 if i lies on a cycle of the kept graph (i has a kept bond whose ends stay connected when that bond is removed), else 0;
 *     id_0(i) = mix(mix(mix(mix(type_i, charge_i), d_i), h_i), c_i)      (type and charge as the unsigned bytes of the record)
 *   Iteration, r = 1 .. R, for every kept atom in every round:
 *     id_r(i) = mix(mix(id_{r-1}(i), r), sum over kept neighbours j of mix(id_{r-1}(j), bond_ij))
 *   Environments: ball_0(i) = {i}, ball_r(i) = ball_{r-1}(i) plus its kept neighbours; E_r(i), r >= 1, is the set of kept bonds with an end
 *     in ball_{r-1}(i).
 *   Features: F_0 = { id_0(i) }.  For r >= 1 the environment (i, r) is NEW when E_r(i) is not empty and differs from E_s(j) for every kept j
 *     and every 1 <= s < r; F_r holds one value per distinct bond set among the new environments of layer r, the smallest id_r(i) over the
 *     environments that share the set.  The fingerprint is the SET F_0 u ... u F_R, at most 29 (R + 1) values.  It is invariant under
 *     renaming atoms by construction: there is no atom order and no "dead atom" chain as in RDKit's sequential duplicate removal - this
 *     is ECFP's duplicate-environment rule stated order-free.  Folded to n_bits the set is { f mod n_bits }.
 * Deviations from the reference's number:
 *   - the records hold Kekule orders 1..3 instead of aromatic bonds: the two Kekule drawings of o-xylene share 5 of their 10 + 10 features
 *     at R = 2;
 *   - RDKit's own invariant hash and fold are not reproduced (bit-for-bit parity is unpinned: RDKit cannot be run where this project
 *     runs), so values differ where the collisions of a 2048-bit fold differ;
 *   - drop_h = 1 is the reference's SMILES route: heavy atoms only, with the hydrogen count in the invariant.
 * Method: an atom per lane, 32-bit atom masks.  c_i from the components of the kept graph without atom i (mask squaring): i is on a cycle
 * iff two of its neighbours share a component.  E(B), the bonds with an end in the atom set B, is represented by the largest atom set with
 * the same bonds, B plus every kept atom all of whose neighbours are in B, so two environments are compared as two masks.
 *
 * ds_morgan_records (one record table, as ds_graph_hash_records):
 *   ids [P,116] u64  the distinct features of molecule p in ascending unsigned order, the remaining slots 0
 *   count [P]   i32  how many there are
 * ds_morgan_similarity_records (record pairs):
 *   n_prb, n_ref i32  sizes of the two sets after folding to n_bits (n_bits = 0: unfolded)
 *   common       i32  size of their intersection: Tanimoto = common / (n_prb + n_ref - common), cosine = common / sqrt(n_prb n_ref)
 *   status       u8   DS_MORGAN_OK, or DS_MORGAN_INVALID: ref_index outside [0, M), nothing is read, the three counts are -1
 * drop_h outside {0, 1}, radius outside [0, DS_MORGAN_MAX_RADIUS] and an n_bits that is neither 0 nor a power of two in
 * [64, DS_MORGAN_MAX_BITS] are DS_ERR_ARG.  Every loop of the kernels is bounded by the atom count, the radius or the 116 slots: a malformed
 * record (dense bond bytes, garbage in the lower triangle or beyond n) ends with the value the definition gives. */
#define DS_MORGAN_MAX_RADIUS 3
#define DS_MORGAN_MAX_FEATURES 116    /* 29 * (3 + 1) */
#define DS_MORGAN_MAX_BITS 4096
#define DS_MORGAN_OK 0
#define DS_MORGAN_INVALID 3
int ds_morgan_records(const uint8_t* rec, const int32_t* n, int64_t P, int32_t drop_h, int32_t radius, uint64_t* ids, int32_t* count,
                      void* stream);
int ds_morgan_similarity_records(const uint8_t* prb_rec, const int32_t* prb_n, int64_t P, const uint8_t* ref_rec, const int32_t* ref_n, int64_t M,
                                 const int64_t* ref_index, int32_t drop_h, int32_t radius, int32_t n_bits, int32_t* common, int32_t* n_prb,
                                 int32_t* n_ref, uint8_t* status, void* stream);

/* Bond lengths, bond angles and dihedral angles of every record, sorted into caller-listed substructure classes: the sample lists behind the
 * reference's "Metric-Align" line (evaluation/cal_geometry.py:14-216 on the unsanitised molecules of evaluation/stability.py:86-120, without
 * RDKit).  One wave per record, an atom per lane; record table, counts, bonds, alignment and P are those of "record pairs" above.  A bond is
 * an atom pair i < j below n whose bond byte o is > 0; N(i) are the atoms bonded to i; type_i is the type byte.  All n atoms count, hydrogens
 * included; the formal charge plays no part; all fragments count.
 *   Bonds      every bond i < j.  Value |x_i - x_j|, in the units of the record's positions.  Fields (type_i, o, type_j).
 *   Angles     every centre c and unordered pair {a, b} of N(c), each once.  With u = x_a - x_c, v = x_b - x_c the value is
 *              acos(clamp(u.v / sqrt(|u|^2 |v|^2), -1, 1)) in degrees, in [0, 180].  Fields (type_a, o_ac, type_c, o_cb, type_b).
 *   Dihedrals  every bond i < j as the middle, every a in N(i) \ {j}, every b in N(j) \ {i}, each (a, i, j, b) once; a == b (a three-ring) is
 *              included, as the reference's loops include it (cal_geometry.py:116-142).  With b1 = x_i - x_a, b2 = x_j - x_i, b3 = x_b - x_j,
 *              n1 = b1 x b2, n2 = b2 x b3 the value is atan2(((n1 x n2).b2) / |b2|, n1.n2) in degrees; rounded to fp32, a value <= -180 becomes
 *              +180, so the range is (-180, 180].  Fields (type_a, o_ai, type_i, o_ij, type_j, o_jb, type_b).
 *   Classes    one int32 per class and at most DS_GEOM_MAX_CLASSES per kind: the fields in 4-bit groups, the first field in bits 0..3, the
 *              next in bits 4..7 and so on (3, 5 or 7 groups; the bits above them 0).  An entry belongs to the first class of its kind's
 *              table whose code equals its fields read forwards or backwards ("up to reversal"); an entry of no class is dropped.  A type
 *              byte or a bond byte above 15 has no code and matches nothing.
 *   Values     fp64 inside (positions widened to fp64, every product and sum rounded on its own: no fused multiply-add, so a value does not
 *              depend on the direction an entry is read in), rounded once to fp32.  An entry of a listed class whose value is undefined or
 *              not finite - coincident atoms, |u|^2 |v|^2 = 0, a zero n1 or n2 at a collinear dihedral, a non-finite coordinate - is not
 *              emitted; `skipped` counts these.
 *   Order      within a record: by lane - the lower atom i of a bond, the centre c of an angle, the lower middle atom i of a dihedral - then
 *              lexicographic in (j), (a, b), (j, a, b); a lane's position comes from a wave prefix sum: the output is bit-identical run to run.
 * The output size depends on the data (29 fully bonded atoms: 406 bonds, 10 962 angles, 295 974 dihedrals), so two entry points walk the same
 * enumeration:
 *   ds_geometry_count_records   counts [P,3] i32 (bonds, angles, dihedrals emitted by record p), skipped [P] i32
 *   ds_geometry_fill_records    offsets [P,3] i64: where record p's entries of each kind start (the caller's exclusive prefix sum of counts
 *                               over p); total_* : the length of each kind's output; per kind value [total] f32 and cls [total] u8 (the class's
 *                               position in its table).  An index at or beyond `total` is never written.  A kind with total 0 takes NULLs.
 * DS_ERR_ARG in the order of "record pairs": a class count outside [0, DS_GEOM_MAX_CLASSES] or a negative total with the sizes; then, for
 * P > 0, a NULL table with a non-zero class count, a NULL output (counts, skipped; offsets, value / cls of a kind with total > 0).
 * Two deviations from the reference's number:
 *   - Angle multiplicity.  The reference counts an angle once per bond whose END atom is the centre (get_bond_pairs, cal_geometry.py:46-59):
 *     0, 1 or 2 times, depending on the atom numbering and on RDKit's begin / end of each bond, which a record does not hold for the test
 *     molecules.  Here every angle counts once, which makes the sample lists invariant under renaming atoms.
 *   - Parity with RDKit's GetAngleDeg / GetDihedralDeg is unpinned: RDKit cannot be run where this project runs.  The global sign convention
 *     of the dihedral cancels in the metric, because both sides go through the same kernel. */
#define DS_GEOM_MAX_CLASSES 32
int ds_geometry_count_records(const uint8_t* rec, const int32_t* n, int64_t P, const int32_t* bond_cls, int32_t n_bond_cls,
                              const int32_t* angle_cls, int32_t n_angle_cls, const int32_t* dihedral_cls, int32_t n_dihedral_cls,
                              int32_t* counts, int32_t* skipped, void* stream);
int ds_geometry_fill_records(const uint8_t* rec, const int32_t* n, int64_t P, const int32_t* bond_cls, int32_t n_bond_cls,
                             const int32_t* angle_cls, int32_t n_angle_cls, const int32_t* dihedral_cls, int32_t n_dihedral_cls,
                             int64_t total_bond, int64_t total_angle, int64_t total_dihedral, const int64_t* offsets,
                             float* bond_value, uint8_t* bond_class, float* angle_value, uint8_t* angle_class,
                             float* dihedral_value, uint8_t* dihedral_class, void* stream);

/* Maximum mean discrepancy of 1-D sample sets with a sum of Gaussian kernels, many (source, target) pairs per call: compute_mmd of
 * evaluation/mmd.py:6-63.  Class c compares x[x_off[c] .. x_off[c+1]) (ns source samples) with y[y_off[c] .. y_off[c+1]) (nt target samples);
 * z is their concatenation, N = ns + nt.
 *   bandwidth = sum over all i, j of (z_i - z_j)^2 / (N^2 - N), or fix_sigma when that is not 0.  In one dimension the sum is 2 N times the
 *               centred second moment, so bandwidth = 2 sum_i (z_i - mean)^2 / (N - 1), taken in fp64 (two passes: mean, then the moment);
 *   bw_k      = bandwidth / kernel_mul^(kernel_num / 2, rounded down) * kernel_mul^k,  k = 0 .. kernel_num - 1;
 *   XX = sum_k sum over i, j in the source (the diagonal included) of exp(-(x_i - x_j)^2 / bw_k) / ns^2, YY alike over the target / nt^2,
 *   XY over source x target / (ns nt);  mmd = XX + YY - 2 XY.
 * out [C,5] f64 = (mmd, XX, YY, XY, bandwidth); status [C] u8:
 *   DS_MMD_OK       a bandwidth that is 0 (all samples identical) or not finite gives NaN in mmd, XX, YY and XY, as the reference does;
 *   DS_MMD_EMPTY    ns = 0 or nt = 0: the five outputs are NaN;
 *   DS_MMD_INVALID  offsets that decrease or leave [0, Nx] / [0, Ny], or more than DS_MMD_MAX_SAMPLES samples on a side: nothing of the class
 *                   is read, the five outputs are NaN.
 * Pairs are evaluated in fp32 (d = x_i - y_j, exp2(d^2 * (-log2 e / bw_k)) on v_exp_f32), summed per lane and bandwidth in fp32 over 64
 * terms, then in fp64.  With kernel_mul = 2 and kernel_num <= 5 one exponential serves every bandwidth (exp(-d^2 / bw_k) is the square of
 * exp(-d^2 / bw_(k+1)); at most four squarings, each of which doubles the relative error).
 * XX and YY visit the upper triangle of DS_MMD_TILE x DS_MMD_TILE tiles and double the tiles off the diagonal.  Workgroup g of a class and term
 * takes tiles g, g + DS_MMD_CHUNKS, ... and leaves one fp64 partial in the workspace; a last kernel adds the partials in index order: no
 * floating-point atomics, bit-identical from run to run.  Stream-ordered, never synchronises.
 * workspace: caller-owned device memory, 8-byte aligned, at least ds_mmd_1d_workspace_bytes(C) bytes (a pure host function), private layout.
 * DS_ERR_ARG: C outside [0, DS_MMD_MAX_CLASSES], Nx or Ny outside [0, 2^31 - 1], kernel_num outside [1, DS_MMD_MAX_KERNELS], a kernel_mul that
 * is not finite and > 0, a fix_sigma that is not finite and >= 0; then, for C > 0 (C = 0 launches nothing): a NULL x_off, y_off, out, status or
 * workspace, a NULL x with Nx > 0 or y with Ny > 0, a workspace that is too small or not 8-byte aligned. */
#define DS_MMD_TILE 256
#define DS_MMD_CHUNKS 128
#define DS_MMD_MAX_SAMPLES 1048576    /* 1 << 20 per side and class */
#define DS_MMD_MAX_KERNELS 8
#define DS_MMD_MAX_CLASSES 65535
#define DS_MMD_OK 0
#define DS_MMD_EMPTY 1
#define DS_MMD_INVALID 2
int ds_mmd_1d_workspace_bytes(int64_t n_classes, int64_t* bytes);
int ds_mmd_1d_segments(const float* x, const int64_t* x_off, int64_t Nx, const float* y, const int64_t* y_off, int64_t Ny, int64_t n_classes,
                       double kernel_mul, int32_t kernel_num, double fix_sigma, void* workspace, int64_t workspace_bytes, double* out,
                       uint8_t* status, void* stream);

/* SpecFormer pieces that are not plain GEMMs (specformer.py:385-425 residual-score attention; :119 LayerNorm).
 * qkv [B,L,3*heads*dk]; out [B,L,heads*dk]; scores: B*heads*L*L floats of caller-owned scratch that carries the
 * pre-softmax scores from layer to layer (has_prev = 0 on the first layer); its layout ([b][h][key][query]) is private. */
int ds_spec_attention(const float* qkv, float* scores, float* out, int B, int L, int heads, int dk, float scale,
                      int has_prev, void* stream);
int ds_layernorm_affine(const float* x, const float* gamma, const float* beta, float* y, int rows, int cols,
                        float eps, void* stream);

/* Measurement hook (bench.py roofline leg): time every `every`-th launch of one block-stage kernel with HIP events
 * recorded on the launch stream.  kernel: 0 edge_geom, 1 node_qkv, 2 attn_fused, 3 node_update, 4 edge_update,
 * 5 equi_pairs (6 is unused since the attention kernels were fused); kernel < 0 disables.  ds_profile_read synchronises the recorded events, returns the summed
 * duration and the sample count, and resets the counters.  Process-global instrumentation state; off by default. */
int ds_profile_config(int kernel, int every, int max_samples);
int ds_profile_read(double* total_ms, int64_t* samples);

/* Position-sensitive 64-bit checksum of a list of fp32 device tensors (wrap-around sum of bits(x) * odd(hash(index)) + index over
 * the concatenation): what the drop-in DMT.forward uses to notice that its packed weights are stale after an in-place edit that
 * leaves Tensor._version untouched (models/ema.py:55,77 write through .data).  ptrs [n] device array of device pointers,
 * prefix [n+1] device int64 element offsets of each tensor in the concatenation, out device uint64 (zeroed here). */
int ds_fingerprint(const float* const* ptrs, const int64_t* prefix, int32_t n, uint64_t* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DIFFSPECTRA_HIP_H */
