// diffspectra_amd - bond orders from distances, shared by ds_check_stability (ds_sampler.hip) and the valence analytics on result records
// (ds_valence.hip): the tables of evaluation/bond_analyze.py:5-45 for H, C, N, O, F (pm; 0 = no such bond), the allowed valences of
// stability.py:61-70, and get_bond_order with the roundings both kernels must share to give equal orders on equal positions.
#pragma once
#include <hip/hip_runtime.h>

namespace ds_bonds {

// (static: every source that includes this holds its own copy, as ds_sampler.hip held its own before)
static __constant__ int c_bond1[5][5] = {{74, 109, 101, 96, 92}, {109, 154, 147, 143, 135}, {101, 147, 145, 140, 136},
                                  {96, 143, 140, 148, 142}, {92, 135, 136, 142, 142}};
static __constant__ int c_bond2[5][5] = {{0, 0, 0, 0, 0}, {0, 134, 129, 120, 0}, {0, 129, 125, 121, 0}, {0, 120, 121, 121, 0}, {0, 0, 0, 0, 0}};
static __constant__ int c_bond3[5][5] = {{0, 0, 0, 0, 0}, {0, 120, 116, 113, 0}, {0, 116, 110, 0, 0}, {0, 113, 0, 0, 0}, {0, 0, 0, 0, 0}};
static __constant__ int c_valence[5] = {1, 4, 3, 2, 1};

// 100 |r| in fp32, every operation rounded on its own (no fused multiply-add): the number the thresholds are compared with
__device__ __forceinline__ float scaled_distance(float dx, float dy, float dz) {
  return __fmul_rn(__fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz))), 100.0f);
}

// get_bond_order: single below L1 + 10, then double below L2 + 5, then triple below L3 + 3; ta, tb in 0..4
__device__ __forceinline__ int order_of(int ta, int tb, float d) {
  int order = 0;
  if (d < (float)(c_bond1[ta][tb] + 10)) {
    order = 1;
    if (c_bond2[ta][tb] != 0 && d < (float)(c_bond2[ta][tb] + 5)) {
      order = 2;
      if (c_bond3[ta][tb] != 0 && d < (float)(c_bond3[ta][tb] + 3)) order = 3;
    }
  }
  return order;
}

}  // namespace ds_bonds
