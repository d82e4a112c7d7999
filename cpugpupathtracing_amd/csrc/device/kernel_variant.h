// kernel_variant.h -- the feature ladder of the render kernels and how a kernel level is encoded.  Plain C++, no HIP: constants and constexpr
// functions for host and device code alike.
//
// The lobe level ("lobe level" is the public word: include/cpugpupt_abi.h) is the int template parameter LOBES of shade_bounce, brute_bounce,
// brute_level, wf_shade and shade_samples_kernel.  The rungs are cumulative -- a rung carries everything below it -- so that a feature adds
// one instantiation per table entry and does not double the tables:
//   0 kLobesMirror          the reference's lobes: no rough lobe, the mirror-only code;
//   1 kLobesRoughSpecular   + the rough specular lobe (ggx_sample): the scene has a material with roughness > 0;
//   2 kLobesRoughDielectric + the rough dielectric lobe (rough_glass_sample): it has one with a transmission roughness > 0 (5.11);
//   3 kLobesSmoothNormals   + get_hit's SMOOTH: it has an object with smooth normals (5.14);
//   4 kLobesTransforms      + get_hit's XFORM and the trace side's: it has an object with a transform (5.16).
// The megakernel and the persistent kernel take a kernel level: the lobe level, or kLobeLevels + the lobe level with the objects reached
// through the top-level tree (cgpt_set_top_level(1)).  The wavefront pipeline's shade kernels take the lobe level itself
// and its trace kernels the tree as a flag.
#pragma once

namespace cgpt {

constexpr int kLobesMirror = 0, kLobesRoughSpecular = 1, kLobesRoughDielectric = 2, kLobesSmoothNormals = 3, kLobesTransforms = 4;
constexpr int kLobeLevels = 5;

constexpr bool HasRoughSpecular(int lobes) { return lobes >= kLobesRoughSpecular; }
constexpr bool HasRoughDielectric(int lobes) { return lobes >= kLobesRoughDielectric; }
constexpr bool ReadsSmoothNormals(int lobes) { return lobes >= kLobesSmoothNormals; }
constexpr bool HonoursTransforms(int lobes) { return lobes >= kLobesTransforms; }

// the lowest rung that carries everything the scene has
constexpr int LobeLevel(bool rough_specular, bool rough_dielectric, bool smooth_normals, bool transforms)
{
    return transforms ? kLobesTransforms : smooth_normals ? kLobesSmoothNormals : rough_dielectric ? kLobesRoughDielectric : rough_specular ? kLobesRoughSpecular : kLobesMirror;
}

constexpr int kKernelLevels = 2 * kLobeLevels;
constexpr int KernelLevel(int lobes, bool tree) { return tree ? kLobeLevels + lobes : lobes; }
constexpr bool ThroughTree(int level) { return level >= kLobeLevels; }
constexpr int LobeOf(int level) { return ThroughTree(level) ? level - kLobeLevels : level; }

// ---- the truth table ------------------------------------------------------------------------------------------------------------------------
namespace variant_check {
constexpr int Predicates(int l) { return (HasRoughSpecular(l) ? 1 : 0) | (HasRoughDielectric(l) ? 2 : 0) | (ReadsSmoothNormals(l) ? 4 : 0) | (HonoursTransforms(l) ? 8 : 0); }
constexpr bool Cumulative(int l) { return l == 0 || ((Predicates(l) & Predicates(l - 1)) == Predicates(l - 1) && Predicates(l) != Predicates(l - 1) && Cumulative(l - 1)); }
constexpr bool RoundTrip(int l) { return l < 0 || (LobeOf(KernelLevel(l, false)) == l && LobeOf(KernelLevel(l, true)) == l && !ThroughTree(KernelLevel(l, false)) && ThroughTree(KernelLevel(l, true)) && KernelLevel(l, false) < kKernelLevels && KernelLevel(l, true) < kKernelLevels && RoundTrip(l - 1)); }
static_assert(Predicates(kLobesMirror) == 0 && Predicates(kLobesRoughSpecular) == 1 && Predicates(kLobesRoughDielectric) == 3 && Predicates(kLobesSmoothNormals) == 7 && Predicates(kLobesTransforms) == 15,
              "each rung's predicates");
static_assert(kLobesTransforms == kLobeLevels - 1 && Cumulative(kLobeLevels - 1), "every rung keeps the rungs below it and adds one feature");
static_assert(RoundTrip(kLobeLevels - 1), "LobeOf(KernelLevel(l, t)) == l and ThroughTree(KernelLevel(l, t)) == t for all ten kernel levels");
static_assert(LobeLevel(false, false, false, false) == kLobesMirror && LobeLevel(true, false, false, false) == kLobesRoughSpecular && LobeLevel(true, true, false, false) == kLobesRoughDielectric &&
              LobeLevel(false, true, false, false) == kLobesRoughDielectric && LobeLevel(true, false, true, false) == kLobesSmoothNormals && LobeLevel(false, false, false, true) == kLobesTransforms &&
              LobeLevel(true, true, true, true) == kLobesTransforms, "the scene's flags pick the lowest rung that carries them all");
// the CGPT_* macros that fill the kernel tables (path_kernels.hip, persistent_kernel.hip, wavefront_kernels.hip, shade_probe.hip) list the levels
// by hand: a new rung is added to each of them
static_assert(kLobeLevels == 5 && kKernelLevels == 10, "list the new level in every kernel table");
}  // namespace variant_check

}  // namespace cgpt
