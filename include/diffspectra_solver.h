/* diffspectra_solver.h - the multistep solver update of the sampling library (libdiffspectra_hip.so): DDIM and DPM-Solver++(2M) in its ODE and
 * SDE form (Lu et al., "DPM-Solver++", 2022) for the data-prediction model, beside the ancestral update of diffspectra_hip.h, which stays as
 * it is.  Plain C, as the other headers; read on the Python side by diffspectra_amd/abi.py (abi.SOLVER) and bound by engine.load_library().
 * (Build extension: the reference ships the ancestral sampler only.)
 *
 * One step is one table row (a, b, c, d) applied to the state x, this step's prediction pred and the previous step's prediction hist:
 *     x_mean = a*x + b*pred + c*hist          x <- x_mean + (d*noise)*temperature
 * on x [B,N,9] and edge_x [B,N,N,2] alike.  The host computes the rows in fp64 (sampling.solver_table): with h = lambda_{i+1} - lambda_i,
 * lambda = log(alpha/sigma), r = h_{i-1}/h_i, E1 = -expm1(-h), E2 = -expm1(-2h):
 *     ddim          a = sigma_{i+1}/sigma_i           k = alpha_{i+1} E1   b = k                c = 0          d = 0
 *     dpmpp_2m      a = sigma_{i+1}/sigma_i           k = alpha_{i+1} E1   b = k (1 + 1/(2r))   c = -k/(2r)    d = 0
 *     sde_dpmpp_2m  a = sigma_{i+1}/sigma_i e^{-h}    k = alpha_{i+1} E2   b = k (1 + 1/(2r))   c = -k/(2r)    d = sigma_{i+1} sqrt(E2)
 * The ancestral update (ds_sampler_step) is the first-order row of sde_dpmpp_2m: (c_x, c_pred, sigma) = (a, k, d).
 *
 * Noise, masks and launch shape are those of ds_sampler_step / ds_sampler_step_philox: one workgroup per molecule, masked N(0,1), position
 * noise CoM-projected per molecule, one draw per unordered atom pair and channel written to (i,j) and (j,i), Philox counter = (element,
 * draw = step + 1, mol_id, kind), key = seed.  Only the valid entries of x, edge_x, x_mean, edge_mean (and of the history, where it is
 * written) are touched.
 *   c == 0  hist / edge_hist are not read (0 * NaN never reaches the output) and may be NULL; c != 0 with either NULL is DS_ERR_ARG.
 *   d == 0  no noise is generated or read: no Philox, no Box-Muller, no raw_* load; raw_pos / raw_feat / raw_edge may be NULL (with d != 0
 *           a NULL one is DS_ERR_ARG).
 * edge_x, edge_pred, edge_hist and edge_mean are read and written two channels at a time: they must be 8-byte aligned (DS_ERR_ARG). */
#ifndef DIFFSPECTRA_SOLVER_H
#define DIFFSPECTRA_SOLVER_H

#include <stdint.h>

#include "diffspectra_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DS_SOLVER_ROW 8              /* floats per row of the device table: (a, b, c, d, noise_level, 0, 0, 0) - 32-byte rows */

/* Noise from the three randn draws of ds_sampler_step: raw_pos [B,N,3], raw_feat [B,N,6], raw_edge [B,2,N,N]. */
int ds_solver_step(const ds_layout* L, float a, float b, float c, float d, float temperature,
                   float* x, float* edge_x, const float* pred, const float* edge_pred, const float* hist, const float* edge_hist,
                   const float* raw_pos, const float* raw_feat, const float* raw_edge, float* x_mean, float* edge_mean, void* stream);

/* Noise generated in the kernel, as ds_sampler_step_philox (mol_id: device int64 [B]). */
int ds_solver_step_philox(const ds_layout* L, float a, float b, float c, float d, float temperature, uint64_t seed, int32_t step,
                          const int64_t* mol_id, float* x, float* edge_x, const float* pred, const float* edge_pred,
                          const float* hist, const float* edge_hist, float* x_mean, float* edge_mean, void* stream);

/* Graph-replayable form, as ds_step_begin + ds_sampler_step_philox_dev: the launch sequence [ds_solver_step_begin, ds_forward,
 * ds_solver_step_philox_dev] has constant arguments.
 *   table [S, DS_SOLVER_ROW] device floats; step device int32: ds_solver_step_begin increments it (it must hold i-1 before iteration i)
 *   and fills noise_level[0..B) with table[*step][4]; ds_solver_step_philox_dev reads its row and the draw index from *step.
 *   hist / edge_hist (required) are the solver's own history: every thread reads the old value of an element (when c != 0) and then
 *   writes this step's prediction over it, so pred may be a buffer that the next ds_forward overwrites in place. */
int ds_solver_step_begin(const float* table, int32_t n_steps, int32_t* step, int32_t B, float* noise_level, void* stream);
int ds_solver_step_philox_dev(const ds_layout* L, const float* table, const int32_t* step, float temperature, uint64_t seed,
                              const int64_t* mol_id, float* x, float* edge_x, const float* pred, const float* edge_pred,
                              float* hist, float* edge_hist, float* x_mean, float* edge_mean, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DIFFSPECTRA_SOLVER_H */
