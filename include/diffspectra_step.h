/* diffspectra_step.h - the uniform-step entry points of the sampling library (libdiffspectra_hip.so): the denoiser forward of
 * diffspectra_hip.h for callers whose B noise levels are all EQUAL, as an ancestral sampler's are (one noise level per step:
 * sampling.py `vec_t = ones(B) * t`, ds_step_begin).  time_mlp (sinusoid features, Linear + GELU, Linear) then has one distinct input
 * row, so it is evaluated once per call instead of B times; `+ ctx_emb`, SiLU and the adaLN GEMM stay per molecule.  Plain C, as the
 * other headers; read on the Python side by diffspectra_amd/abi.py (abi.STEP) and bound by engine.load_library().
 *
 * Contract: noise_level is a DEVICE pointer of which only element 0 is read (so a captured launch sequence that refills it with
 * ds_step_begin replays unchanged); every output is bit-identical to the per-molecule entry point called with that value in all B
 * entries.  A caller whose noise levels may differ (training, DMT.forward) uses ds_stage_time / ds_forward.
 * (Build extension: the reference evaluates time_mlp on all B rows.) */
#ifndef DIFFSPECTRA_STEP_H
#define DIFFSPECTRA_STEP_H

#include <stdint.h>

#include "diffspectra_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ds_stage_time with the time MLP on one row: leaves ws->temb_silu and ws->ada as ds_stage_time does on a filled noise-level vector. */
int ds_stage_time_uniform(const ds_weights* w, const ds_layout* L, ds_workspace* ws, const float* noise_level, const float* ctx_emb,
                          void* stream);

/* ds_forward with that prologue; arguments, block schedules (one or two streams) and threading rule as ds_forward. */
int ds_forward_uniform(const ds_weights* w, const ds_layout* L, ds_workspace* ws, const float* xh, const float* edge_x,
                       const float* cond_x, const float* cond_edge_x, const float* noise_level, const float* ctx_emb, float* out_xh,
                       float* out_edge, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DIFFSPECTRA_STEP_H */
