// minmax_std.h -- std::min / std::max as the reference's Vec3Min / Vec3Max evaluate them (ref: MathLib.h:95-96), for host and device.
// The comparison direction matters: a NaN operand never replaces the first argument and a tie keeps it, so the sign of a zero
// bound is the one the sequential fold leaves.  fminf / fmaxf (v_min_f32 / v_max_f32) differ on both counts.
#pragma once

namespace cgpt {
__device__ __host__ inline float min_std(float a, float b) { return (b < a) ? b : a; }   // std::min(a,b), ref: MathLib.h:95
__device__ __host__ inline float max_std(float a, float b) { return (a < b) ? b : a; }   // std::max(a,b), ref: MathLib.h:96
}  // namespace cgpt
