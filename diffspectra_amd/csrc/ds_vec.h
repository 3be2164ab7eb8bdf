// diffspectra_amd - the fp64 three-vector of the stereo perception (ds_stereo.hip, ds_key.hip): positions are a record's fp32 values widened to
// fp64, every geometric quantity of a site is formed from these operations.
#pragma once
#include <hip/hip_runtime.h>

namespace ds_vec {

struct Vec { double x, y, z; };
__device__ __forceinline__ Vec operator-(Vec a, Vec b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ Vec operator*(Vec a, double s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ double dot(Vec a, Vec b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ Vec cross(Vec a, Vec b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ bool finite(Vec a) { return isfinite(a.x) && isfinite(a.y) && isfinite(a.z); }
__device__ __forceinline__ Vec widen(const float (&p)[3]) { return {(double)p[0], (double)p[1], (double)p[2]}; }

}  // namespace ds_vec
