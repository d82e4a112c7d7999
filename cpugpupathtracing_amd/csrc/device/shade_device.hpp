// shade_device.hpp -- one bounce of TracePathAdvanced (ref: Source/Main.cpp:404-573) as a device function shared by the
// megakernel and the wavefront shade kernel.  Given the closest-hit record of the extend ray it performs, in the
// reference's order (RNG draw order: SURVEY Appendix C): hit reconstruction, emissive add, NEE light sample (-> shadow ray
// + pending contribution), Russian roulette, lobe choice (mirror / dielectric + Beer / diffuse) -> next ray.
// The shadow ray draws no random numbers, so computing the next ray before the shadow ray is traced changes nothing.
#pragma once
#include <hip/hip_runtime.h>

#include "device_scene.h"
#include "kernel_variant.h"
#include "rt_device.hpp"

namespace cgpt {
namespace dev {

struct Hit { V3 pos, normal; uint32_t mat; };

// The interpolated shading normal of a hit at P on triangle (p0, p1, p2) with vertex normals (n0, n1, n2), ray direction d (DESIGN.md 5.14;
// tests/smooth_ref.py states the same operations in numpy and is the specification).  float32, no contraction, in this order:
//  1. n0, n1, n2 bitwise equal -> n0, nothing else computed (decided by the caller, before the position records are read);
//  2. e1 = p1 - p0, e2 = p2 - p0, w = P - p0, g = cross(e1, e2), gg = dot(g, g);
//  3. u = dot(cross(w, e2), g) / gg, v = dot(cross(e1, w), g) / gg: the projection of P onto the triangle's plane, independent of d;
//  4. m = (1 - u - v) n0 + u n1 + v n2, l2 = dot(m, m); !(l2 > 1e-12) (NaN, a degenerate triangle, cancelling normals) -> n0; else ns = m / sqrt(l2);
//  5. the side stays the geometry's: g is flipped so that dot(g, ns) >= 0; if d sees ns and g from different sides (dot(d, ns) dot(d, g) < 0)
//     or grazes ns (dot(d, ns) == 0), the normal is normalize(g) -- the integrator decides inside / outside and the reflection side from
//     dot(d, normal), and that sign must be the real surface's.
__device__ __forceinline__ V3 smooth_normal(V3 p0, V3 p1, V3 p2, V3 n0, V3 n1, V3 n2, V3 P, V3 d)
{
    const V3 e1 = p1 - p0, e2 = p2 - p0, w = P - p0;
    V3 g = cross(e1, e2);
    const float gg = dot(g, g);
    const float u = dot(cross(w, e2), g) / gg;
    const float v = dot(cross(e1, w), g) / gg;
    const V3 m = (1.0f - u - v) * n0 + u * n1 + v * n2;
    const float l2 = dot(m, m);
    if (!(l2 > 1e-12f)) return n0;
    const float len = sqrtf(l2);
    V3 ns = mk(m.x / len, m.y / len, m.z / len);
    if (dot(g, ns) < 0.0f) g = -g;
    const float dn = dot(d, ns);
    if (dn * dot(d, g) < 0.0f || dn == 0.0f) ns = normalize(g);
    return ns;
}

// GetRayHitResult (ref: Main.cpp:325-338): flat shading normal = v0.normal of the hit triangle (SURVEY A-8).  A triangle object's
// normal is its own record's (TriangleNormal, ref: Primitives.cpp:308-321): ray.tri may be left over from an earlier mesh's hit.
// SMOOTH: the scene has an object with DevObject.smooth set (cgpt_scene_update_smooth_normals); a hit on such a mesh or triangle object
// gets smooth_normal() above.  The instantiations without it read neither the flag nor the {n1, n2} records: the code they had.
// XFORM: the scene has an object with the transform flag set (cgpt_scene_update_transforms; rt_device.hpp: has_xform).  The hit position stays o + d t of the world ray.
// The flat normal of a hit on such an object is xform_normal(n0) = normalize(Ainv^T n0) (an untransformed object's v0.normal is still passed
// through unnormalised); with the smooth flag, smooth_normal runs in object space -- P' = o' + d' t, direction d', which keeps its side
// tests' meaning: dot(d', n') = dot(d, Ainv^T n') -- and its result is mapped the same way.
template <bool COUNT, bool SMOOTH = false, bool XFORM = false>
__device__ __forceinline__ Hit get_hit(const DevScene& sc, const Ray& ray, Counters& cnt)
{
    Hit h;
    h.pos = ray.o + ray.d * ray.t;
    const DevObject& obj = sc.objects[ray.obj];
    if (XFORM && (obj.kind == 0u || obj.kind == CGPT_OBJECT_TRIANGLE) && has_xform(sc, ray.obj)) {
        const Xform x = load_xform(sc, ray.obj);
        const uint32_t t = obj.tri_base + (obj.kind == 0u ? ray.tri : 0u);
        const float4 n = sc.tri_normal[t];
        V3 no = mk(n.x, n.y, n.z);
        if (SMOOTH && obj.smooth != 0u) {
            const float4* pair = sc.tri_normal + sc.n_tris_total + 2u * (size_t)t;
            const float4 a = pair[0], b = pair[1];
            const bool same = __float_as_uint(a.x) == __float_as_uint(n.x) && __float_as_uint(a.y) == __float_as_uint(n.y) && __float_as_uint(a.z) == __float_as_uint(n.z) &&
                              __float_as_uint(b.x) == __float_as_uint(n.x) && __float_as_uint(b.y) == __float_as_uint(n.y) && __float_as_uint(b.z) == __float_as_uint(n.z);
            if (!same) {
                V3 oo, od;
                xform_ray(x, ray.o, ray.d, oo, od);
                const float4* rec = sc.tri_orig + 3u * (size_t)t;
                const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2];
                no = smooth_normal(mk(r0.x, r0.y, r0.z), mk(r1.x, r1.y, r1.z), mk(r2.x, r2.y, r2.z), no, mk(a.x, a.y, a.z), mk(b.x, b.y, b.z), oo + od * ray.t, od);
            }
        }
        h.normal = xform_normal(x, no);
        if (COUNT) cnt.hits += obj.kind == 0u ? 1u : 0u;
    } else if (obj.kind == 0u || obj.kind == CGPT_OBJECT_TRIANGLE) {
        const uint32_t t = obj.tri_base + (obj.kind == 0u ? ray.tri : 0u);
        const float4 n = sc.tri_normal[t];
        h.normal = mk(n.x, n.y, n.z);
        if (SMOOTH && obj.smooth != 0u) {
            const float4* pair = sc.tri_normal + sc.n_tris_total + 2u * (size_t)t;
            const float4 a = pair[0], b = pair[1];
            const bool same = __float_as_uint(a.x) == __float_as_uint(n.x) && __float_as_uint(a.y) == __float_as_uint(n.y) && __float_as_uint(a.z) == __float_as_uint(n.z) &&
                              __float_as_uint(b.x) == __float_as_uint(n.x) && __float_as_uint(b.y) == __float_as_uint(n.y) && __float_as_uint(b.z) == __float_as_uint(n.z);
            if (!same) {
                const float4* rec = sc.tri_orig + 3u * (size_t)t;
                const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2];
                h.normal = smooth_normal(mk(r0.x, r0.y, r0.z), mk(r1.x, r1.y, r1.z), mk(r2.x, r2.y, r2.z), h.normal, mk(a.x, a.y, a.z), mk(b.x, b.y, b.z), h.pos, ray.d);
            }
        }
        if (COUNT) cnt.hits += obj.kind == 0u ? 1u : 0u;                      // mesh hits only (ref: Main.cpp:332)
    } else if (obj.kind == 1u) {
        h.normal = normalize(h.pos - mk(obj.sphere_center));                 // ref: Primitives.cpp:153-156
    } else {
        h.normal = mk(obj.plane_normal);                                     // ref: Primitives.cpp:158-161
    }
    h.mat = obj.mat_index;
    return h;
}

struct LightSample { V3 to_light, normal, emission; float distance, area; };

// GetRandomLightSourceForSample (ref: Main.cpp:351-394)
__device__ __forceinline__ LightSample sample_light(const DevScene& sc, uint32_t& rng, V3 hit_pos)
{
    LightSample ls;
    const uint32_t light_obj = sc.lights[random_range(rng, 0u, sc.n_lights - 1u)];
    const DevObject& light = sc.objects[light_obj];
    V3 pos;
    if (light.kind == 0u) {                                                   // mesh light, ref: Main.cpp:360-368
        const uint32_t t = random_range(rng, 0u, light.n_tris - 1u);
        const float4* rec = sc.tri_orig + 3u * (size_t)(light.tri_base + t);
        float4 r0 = rec[0], r1 = rec[1], r2 = rec[2];
        float u0 = random_float(rng);                                         // RandomPointTriangle, ref: Primitives.cpp:170-186
        float u1 = random_float(rng);
        float alpha = u0, beta = u1;
        if (alpha + beta > 1.0f) { alpha = 1.0f - alpha; beta = 1.0f - beta; }
        float gamma = 1.0f - beta - alpha;
        pos = alpha * mk(r0.x, r0.y, r0.z) + beta * mk(r1.x, r1.y, r1.z) + gamma * mk(r2.x, r2.y, r2.z);
        ls.normal = mk(r0.w, r1.w, r2.w);
        ls.area = light.total_area / 2.0f;
    } else {                                                                  // sphere light, ref: Main.cpp:371-380
        V3 c = mk(light.sphere_center);
        V3 to_pos = normalize(hit_pos - c);                                   // RandomPointSphereFacing, ref: Primitives.cpp:214-220
        V3 dir = uniform_hemisphere_sample(rng, to_pos);
        pos = c + light.sphere_radius * dir;
        ls.normal = normalize(pos - c);
        ls.area = 2.0f * kPi * light.sphere_radius_sq;
    }
    ls.to_light = pos - hit_pos;
    ls.distance = length(ls.to_light);
    ls.to_light = normalize(ls.to_light);
    const float4* mp = sc.materials + 4u * (size_t)light.mat_index;
    float4 c2 = mp[2], c3 = mp[3];
    ls.emission = mk(c2.y, c2.z, c2.w) * c3.x;                                // emissive * intensity
    return ls;
}

// The unshadowed contribution of light sample ls to a hit with cosines NdotL, NLdotL (ref: Main.cpp:446-462): the one-sample NEE's
// `pending`, a RIS candidate's c_j.  The caller decides whether the cosines are tested first.
__device__ __forceinline__ V3 nee_unshadowed(const DevScene& sc, const Mat& mat, V3 throughput, const LightSample& ls, float NdotL, float NLdotL,
                                             float diffuse_weight)
{
    const V3 brdf_diffuse = mat.albedo * kInvPi;
    const float solid_angle = (NLdotL * ls.area) / (ls.distance * ls.distance);
    const float light_pdf = 1.0f / solid_angle;
    return throughput * (NdotL / light_pdf) * brdf_diffuse * ls.emission * (float)sc.n_lights * diffuse_weight;
}

// the ray a bounce goes on with: direction dir from the hit, nudged off the surface (ref: Main.cpp:49)
__device__ __forceinline__ Ray next_ray(const Hit& hit, V3 dir) { return make_ray(hit.pos + dir * kNudge, dir, 1e34f); }

// Beer's law over the distance t travelled inside the medium; applied on the way out only (SURVEY A-4)
__device__ __forceinline__ V3 beer_absorption(const Mat& mat, float t)
{
    V3 ab;
    ab.x = expf(-mat.absorption.x * t);
    ab.y = expf(-mat.absorption.y * t);
    ab.z = expf(-mat.absorption.z * t);
    return ab;
}

// BVH-depth debug view of a primary ray (ref: Main.cpp:408-412, 594-597)
__device__ __forceinline__ V3 bvh_depth_colour(const Ray& ray)
{
    return lerp(mk(0.0f, 1.0f, 0.0f), mk(1.0f, 0.0f, 0.0f), (float)ray.bvh_depth / 30.0f);
}

// The smooth dielectric interface (ref: Main.cpp:488-546 and 621-675): sides and indices from dot(normal, d); k < 0 is total internal
// reflection (no draw, dir not set); otherwise one float is drawn against fresnel() and dir is the refracted direction when it is greater,
// else the mirror lobe's.  `inside`: the ray travelled in the medium (Beer's law applies to a refraction out of it).  What each outcome
// does to the path is the integrator's business.
enum : uint32_t { kGlassTir = 0u, kGlassRefract = 1u, kGlassReflect = 2u };
// the interface as the ray meets it: the normal turned against the ray, the cosine, the indices on either side, and k.  A function of the
// ray's direction and the hit alone -- no draw -- so the same ray on the same hit gets the same k (shade_bounce: stuck iterations).
__device__ __forceinline__ float glass_interface(const Mat& mat, const Hit& hit, const Ray& ray, V3& N, float& cosi, float& etai, float& etat, bool& inside)
{
    N = hit.normal;
    cosi = clamp_std(dot(N, ray.d), -1.0f, 1.0f);
    etai = 1.0f; etat = mat.ior;
    inside = true;
    if (cosi < 0.0f) { cosi = -cosi; inside = false; }
    else { float tmp = etai; etai = etat; etat = tmp; N = -N; }
    const float eta = etai / etat;
    return 1.0f - eta * eta * (1.0f - cosi * cosi);
}
__device__ __forceinline__ uint32_t smooth_glass(const Mat& mat, const Hit& hit, const Ray& ray, uint32_t& rng, V3& dir, bool& inside)
{
    V3 N; float cosi, etai, etat;
    const float k = glass_interface(mat, hit, ray, N, cosi, etai, etat, inside);
    if (!(k >= 0.0f)) return kGlassTir;
    const float eta = etai / etat;
    const V3 rd = refract(ray.d, N, eta, cosi, k);
    const float angle_in = dot(ray.d, hit.normal);
    const float angle_out = dot(rd, hit.normal);
    const float Fr = fresnel(angle_in, angle_out, etai, etat);
    if (random_float(rng) > Fr) { dir = rd; return kGlassRefract; }
    dir = reflect(ray.d, hit.normal);
    return kGlassReflect;
}

// ---- rough lobes (kernel_variant.h) -----------------------------------------------------------------------
// Smith L(w) = (-1 + sqrt(1 + alpha^2 tan^2(theta_w))) / 2 of a direction whose cosine to n is z (a2 = alpha^2).
__device__ __forceinline__ float ggx_lambda(float a2, float z)
{
    return 0.5f * (-1.0f + sqrtf(1.0f + a2 * (max_std(0.0f, 1.0f - z * z) / (z * z))));
}

static constexpr float kGgxMinCosSq = 1.17549435e-38f;                       // FLT_MIN: 1 / oz^2 stays finite from here up

// A microfacet normal h from the visible normals of wo = -d (Heitz 2018, JCGT 7(4)) around n, the shading normal turned to face the ray,
// with the two floats u1, u2.  oz = wo.n.  Returns false when wo lies at or below the horizon of n (h is then not set).
__device__ __forceinline__ bool ggx_visible_normal(float u1, float u2, V3 d, V3 normal, float alpha, V3& n, float& oz, V3& h)
{
    n = dot(d, normal) > 0.0f ? -normal : normal;
    const float sign = copysignf(1.0f, n.z);                                  // orthonormal basis around n (Duff et al. 2017)
    const float a = -1.0f / (sign + n.z), b = n.x * n.y * a;
    const V3 tx = mk(1.0f + sign * n.x * n.x * a, sign * b, -sign * n.x);
    const V3 ty = mk(b, sign + n.y * n.y * a, -n.y);
    const V3 wo = -d;
    const float ox = dot(wo, tx), oy = dot(wo, ty);
    oz = dot(wo, n);
    // ... or so close above it that oz^2 is below the smallest normal float (oz < 1.09e-19): ggx_lambda's tan^2 = (1 - oz^2) / oz^2 would be inf
    // and the weight inf / inf.  The lobe's limit there is a weight of 1 on a direction below the horizon: no energy, as for oz <= 0.
    if (!(oz > 0.0f) || !(oz * oz >= kGgxMinCosSq)) return false;
    const V3 vh = normalize(mk(alpha * ox, alpha * oy, oz));                  // stretch wo to the alpha = 1 configuration
    const float lensq = vh.x * vh.x + vh.y * vh.y;
    const V3 t1 = lensq > 0.0f ? mk(-vh.y, vh.x, 0.0f) * (1.0f / sqrtf(lensq)) : mk(1.0f, 0.0f, 0.0f);
    const V3 t2 = cross(vh, t1);
    const float rad = sqrtf(u1), phi = 2.0f * kPi * u2;                       // a point on the projected visible hemisphere
    const float p1 = rad * cosf(phi);
    const float s = 0.5f * (1.0f + vh.z);
    const float p2 = (1.0f - s) * sqrtf(max_std(0.0f, 1.0f - p1 * p1)) + s * (rad * sinf(phi));
    const V3 nh = p1 * t1 + p2 * t2 + sqrtf(max_std(0.0f, 1.0f - p1 * p1 - p2 * p2)) * vh;
    const V3 hl = normalize(mk(alpha * nh.x, alpha * nh.y, max_std(0.0f, nh.z)));   // unstretch
    h = hl.x * tx + hl.y * ty + hl.z * n;
    return true;
}

// Rough specular lobe (HasRoughSpecular): isotropic GGX reflection with the constant Fresnel `albedo` the mirror lobe has.  h is drawn with
// u1, u2 -- the two draws after the lobe choice -- and wi = reflect(-wo, h).  D and the sampling pdf cancel: the estimator's factor is
// G2 / G1 with the height-correlated Smith G2 = 1 / (1 + L(wo) + L(wi)), G1 = 1 / (1 + L(wo)).
// Returns false when wi lies at or below the horizon of n (or wo grazes it): the lobe has no energy there.
__device__ __forceinline__ bool ggx_sample(uint32_t& rng, V3 d, V3 normal, float alpha, V3& wi, float& weight)
{
    const float u1 = random_float(rng);
    const float u2 = random_float(rng);
    V3 n, h; float oz;
    if (!ggx_visible_normal(u1, u2, d, normal, alpha, n, oz, h)) return false;
    wi = reflect(d, h);
    const float iz = dot(wi, n);
    if (!(iz > 0.0f)) return false;
    const float a2 = alpha * alpha;
    const float lambda_o = ggx_lambda(a2, oz);
    const float lambda_i = ggx_lambda(a2, iz);
    weight = (1.0f + lambda_o) / (1.0f + lambda_o + lambda_i);
    return true;
}

// Rough dielectric lobe (HasRoughDielectric, Walter et al. 2007): the smooth lobe's interface with the microfacet normal h in the role of the
// normal.  Sides and indices are the smooth lobe's, from dot(normal, d); h comes from the visible normals with u1, u2; with c = wo.h and
// k = 1 - eta^2 (1 - c^2), a facet with k >= 0 draws one more float against the reference's fresnel() and refracts when it is greater,
// and a facet with k < 0 reflects totally (no draw) -- physical TIR, not the smooth lobe's re-traced ray or black leaf.  The factor is
// G2 / G1 as in ggx_sample, L taken at |w.n|, for the reflected and the refracted w alike; no eta^2 scaling.
// Returns kRoughGlassNone when w lies on the wrong side of n for its kind (or wo grazes it): no energy.
enum : uint32_t { kRoughGlassNone = 0u, kRoughGlassReflect = 1u, kRoughGlassRefract = 2u };
__device__ __forceinline__ uint32_t rough_glass_sample(uint32_t& rng, V3 d, V3 normal, float alpha, float ior, V3& w, float& weight, bool& inside)
{
    const float u1 = random_float(rng);
    const float u2 = random_float(rng);
    float etai = 1.0f, etat = ior;
    inside = !(clamp_std(dot(normal, d), -1.0f, 1.0f) < 0.0f);
    if (inside) { etai = ior; etat = 1.0f; }
    const float eta = etai / etat;
    V3 n, h; float oz;
    if (!ggx_visible_normal(u1, u2, d, normal, alpha, n, oz, h)) return kRoughGlassNone;
    const float dh = dot(d, h), c = -dh;
    const float k = 1.0f - eta * eta * (1.0f - c * c);
    bool refracts = false;
    V3 wt = mk(0.0f);
    if (k >= 0.0f) {
        wt = refract(d, h, eta, c, k);
        const float Fr = fresnel(dh, dot(wt, h), etai, etat);
        refracts = random_float(rng) > Fr;
    }
    w = refracts ? wt : reflect(d, h);
    const float wz = dot(w, n);
    if (refracts ? !(wz < 0.0f) : !(wz > 0.0f)) return kRoughGlassNone;
    const float a2 = alpha * alpha;
    const float lambda_o = ggx_lambda(a2, oz);
    const float lambda_w = ggx_lambda(a2, fabsf(wz));
    weight = (1.0f + lambda_o) / (1.0f + lambda_o + lambda_w);
    return refracts ? kRoughGlassRefract : kRoughGlassReflect;
}

struct PathState {
    V3 throughput, energy;
    uint32_t rng, depth;
    bool is_specular;
};

enum : uint32_t { kBounceTerminate = 1u, kBounceShadow = 2u, kBounceEnergy = 4u, kBounceBruteDone = 8u };   // kBounceEnergy: ps.energy was added to; kBounceBruteDone (wavefront shade): ps.energy is a finished TracePath's radiance
// bits 4-5: the lobe that made the next ray when it is a function of the traced ray and its hit alone (wavefront shade: specular chains)
enum : uint32_t { kBounceChainShift = 4u, kChainReflect = 1u, kChainRefract = 2u, kChainTir = 3u };

// A hit on a light ends the path and draws no number; its emission counts where NEE has not sampled it already (ref: Main.cpp:424-431).
// True: ps.energy was added to.  (wavefront shade calls it too, for an extend ray its probe decides as a hit on a light.)
__device__ __forceinline__ bool add_light_hit(const DevSettings& st, PathState& ps, V3 emissive, float intensity)
{
    if (!st.nee || ps.depth == 0 || ps.is_specular) { ps.energy = ps.energy + ps.throughput * emissive * intensity; return true; }
    return false;
}

// Processes the hit of `ray` (already traced).  On return: `ray` is the next extend ray unless kBounceTerminate is set;
// if kBounceShadow is set, `shadow` / `pending` describe the NEE connection to trace (energy += pending when unoccluded,
// ref: Main.cpp:452-463).  Emissive energy is added here; the final debug-view overrides are applied by the caller.
// LOBES: the lobe level, kernel_variant.h.
// RIS: the NEE light sample is the survivor of M = st.nee > 1 candidates (resampled importance sampling); the
// instantiations without it keep the one-sample code.
template <bool COUNT, int LOBES = 0, bool RIS = false>
__device__ __forceinline__ uint32_t shade_bounce(const DevScene& sc, const DevSettings& st, Ray& ray, PathState& ps, Ray& shadow,
                                                 V3& pending, Counters& cnt)
{
    constexpr bool ROUGH_SPECULAR = HasRoughSpecular(LOBES), ROUGH_DIELECTRIC = HasRoughDielectric(LOBES);
    if (ps.depth == 0 && st.debug_mode == 2u) {                               // BVH-depth view, ref: Main.cpp:408-412
        ps.energy = ps.energy + bvh_depth_colour(ray);
        return kBounceTerminate | kBounceEnergy;
    }
    if (ray.obj == kNoHit) return kBounceTerminate;                           // ref: Main.cpp:415-416

    const Hit hit = get_hit<COUNT, ReadsSmoothNormals(LOBES), HonoursTransforms(LOBES)>(sc, ray, cnt);
    const Mat mat = load_material(sc, hit.mat);
    if (mat.is_light) return add_light_hit(st, ps, mat.emissive, mat.intensity) ? kBounceTerminate | kBounceEnergy : kBounceTerminate;   // ref: Main.cpp:424-431

    uint32_t result = 0;
    const float diffuse_weight = max_std(0.0f, 1.0f - mat.specular - mat.refractivity);
    if (RIS && sc.n_lights > 0 && st.nee && diffuse_weight > 0.001f) {
        // M candidates, each drawn as sample_light draws and weighed by its unshadowed contribution c_j (the one-sample code's `pending`,
        // 0 when a cosine test fails): w_j = c_j.x + c_j.y + c_j.z.  One float u_j follows every candidate's draws, the first and the
        // weightless ones included, and decides the streaming reservoir; a candidate that finds it empty is taken whatever u_j is
        // (random_float can return 1.0f).  The survivor y gets the one shadow ray and pending = c_y * wsum / (M w_y).
        // No early exit and no branch around a draw, so the loop is the same for every lane; but the candidates are serial: the light index
        // of j + 1 comes from the RNG state after j, whose draw count depends on objects[].kind (and ball_sample rejects), so a lane pays
        // about M x the dependent chain lights[] -> objects[] -> materials[] (+ three triangle records for a mesh light) per bounce.
        const uint32_t M = st.nee;
        float wsum = 0.0f, w_y = 0.0f, dist_y = 0.0f;
        V3 c_y = mk(0.0f), dir_y = mk(0.0f);
        for (uint32_t j = 0; j < M; ++j) {
            const LightSample ls = sample_light(sc, ps.rng, hit.pos);
            const float u = random_float(ps.rng);
            const float NdotL = dot(hit.normal, ls.to_light);
            const float NLdotL = dot(ls.normal, -ls.to_light);
            const V3 c = nee_unshadowed(sc, mat, ps.throughput, ls, NdotL, NLdotL, diffuse_weight);
            const float w = (NdotL > 0.0f && NLdotL > 0.0f) ? c.x + c.y + c.z : 0.0f;
            wsum += w;
            if (w > 0.0f && (w_y == 0.0f || u * wsum < w)) { c_y = c; w_y = w; dir_y = ls.to_light; dist_y = ls.distance; }   // w_y == 0: empty
        }
        if (wsum > 0.0f) {
            shadow = make_ray(hit.pos + dir_y * kNudge, dir_y, dist_y - 2.0f * kNudge);
            pending = c_y * (wsum / ((float)M * w_y));
            result |= kBounceShadow;
        }
    } else if (sc.n_lights > 0 && st.nee && diffuse_weight > 0.001f) {        // ref: Main.cpp:439-465
        const LightSample ls = sample_light(sc, ps.rng, hit.pos);
        const float NdotL = dot(hit.normal, ls.to_light);
        const float NLdotL = dot(ls.normal, -ls.to_light);
        if (NdotL > 0.0f && NLdotL > 0.0f) {
            shadow = make_ray(hit.pos + ls.to_light * kNudge, ls.to_light, ls.distance - 2.0f * kNudge);
            pending = nee_unshadowed(sc, mat, ps.throughput, ls, NdotL, NLdotL, diffuse_weight);
            result |= kBounceShadow;
        }
    }

    // Russian roulette on albedo (ref: Main.cpp:468-475); the float is drawn even when p == 1
    if (st.rr) {
        const float p = survival_probability_rr(mat.albedo);
        if (p < random_float(ps.rng)) return result | kBounceTerminate;
        ps.throughput = ps.throughput * mk(1.0f / p);
    }

    float r = random_float(ps.rng);                                           // ref: Main.cpp:478

    // Stuck iterations.  After total internal reflection the reference traces the same ray again (SURVEY A-3) and lands on
    // the same hit: no emissive add (the material is no light), the same NEE decision, the roulette and lobe draws above and -- if the
    // smooth dielectric is drawn again -- the same k < 0, until another lobe is drawn, the roulette ends the path or the depth runs out.
    // Where this material samples no light such an iteration is nothing but those draws, so it runs here, in place: the same draws in the
    // same order, the same throughput * (1 / p), the same depth++, and one IntersectScene call counted.  Whatever r ends the loop goes
    // through the lobes below as it always did.  Not in the counting kernels, which walk every ray the oracle walks.
    bool absorbed = false;
    if (!COUNT && !(sc.n_lights > 0 && st.nee && diffuse_weight > 0.001f)) {
        const bool rough_t = ROUGH_DIELECTRIC && mat.alpha_t > 0.0f;
        V3 N; float cosi, etai, etat; bool inside;
        if (!rough_t && !(r < mat.specular) && r < mat.specular + mat.refractivity && !(glass_interface(mat, hit, ray, N, cosi, etai, etat, inside) >= 0.0f)) {
            while ((int32_t)(ps.depth + 1u) <= st.max_ray_depth) {
                ps.depth++;
                cnt.rays++; cnt.unwalked++;
                absorbed = true;
                if (st.rr) {
                    const float p = survival_probability_rr(mat.albedo);
                    if (p < random_float(ps.rng)) return result | kBounceTerminate;
                    ps.throughput = ps.throughput * mk(1.0f / p);
                }
                r = random_float(ps.rng);
                if (r < mat.specular || !(r < mat.specular + mat.refractivity)) break;
            }
        }
    }

    if (ROUGH_SPECULAR && r < mat.specular && mat.alpha > 0.0f) {                     // rough specular lobe
        V3 gd; float g;
        if (!ggx_sample(ps.rng, ray.d, hit.normal, mat.alpha, gd, g)) return result | kBounceTerminate;   // below the horizon: ends as RR ends it
        ray = next_ray(hit, gd);
        ps.throughput = ps.throughput * (mat.albedo * g);
        ps.is_specular = true;                                                // light hits count, as after the mirror; chain choice 0
    } else if (r < mat.specular) {                                            // mirror, ref: Main.cpp:480-487
        ray = next_ray(hit, reflect(ray.d, hit.normal));
        ps.throughput = ps.throughput * mat.albedo;
        ps.is_specular = true;
        result |= kChainReflect << kBounceChainShift;
    } else if (ROUGH_DIELECTRIC && r < mat.specular + mat.refractivity && mat.alpha_t > 0.0f) {   // rough dielectric lobe
        V3 gd; float g; bool inside;
        const uint32_t kind = rough_glass_sample(ps.rng, ray.d, hit.normal, mat.alpha_t, mat.ior, gd, g, inside);
        if (kind == kRoughGlassNone) return result | kBounceTerminate;       // the wrong side: ends as RR ends it
        ps.throughput = ps.throughput * (mat.albedo * g);
        if (kind == kRoughGlassRefract && inside) ps.throughput = ps.throughput * beer_absorption(mat, ray.t);   // on the way out only, as in the smooth lobe
        ray = next_ray(hit, gd);
        ps.is_specular = true;                                                // chain choice 0
    } else if (r < mat.specular + mat.refractivity) {                         // dielectric, ref: Main.cpp:488-546
        V3 gd; bool inside;
        const uint32_t kind = smooth_glass(mat, hit, ray, ps.rng, gd, inside);
        if (kind == kGlassRefract) {
            ps.throughput = ps.throughput * mat.albedo;
            if (inside) ps.throughput = ps.throughput * beer_absorption(mat, ray.t);
            ray = next_ray(hit, gd);
            ps.is_specular = true;
            result |= kChainRefract << kBounceChainShift;
        } else if (kind == kGlassReflect) {                                   // the same ray as the mirror lobe's
            ray = next_ray(hit, gd);
            ps.throughput = ps.throughput * mat.albedo;
            ps.is_specular = true;
            result |= kChainReflect << kBounceChainShift;
        } else {
            // total internal reflection: the ray is left as it is -- t, obj, tri included -- and is traced again next iteration (SURVEY A-3)
            result |= kChainTir << kBounceChainShift;
        }
    } else {                                                                  // diffuse, ref: Main.cpp:547-570
        V3 dd; float NdotR, pdf;
        if (st.cosine) {
            dd = cosine_weighted_diffuse_reflection(ps.rng, hit.normal);
            NdotR = dot(dd, hit.normal);
            pdf = 1.0f / (2.0f * kPi);                                        // swapped pdfs kept: SURVEY A-7
        } else {
            dd = uniform_hemisphere_sample(ps.rng, hit.normal);
            NdotR = dot(dd, hit.normal);
            pdf = NdotR / kPi;
        }
        ray = next_ray(hit, dd);
        ps.throughput = ps.throughput * ((NdotR / pdf) * (mat.albedo * kInvPi));
        ps.is_specular = false;
    }
    if (absorbed) result &= ~(3u << kBounceChainShift);                       // no longer a chain from the camera that an election could share: choice 0
    ps.depth++;
    if ((int32_t)ps.depth > st.max_ray_depth) result |= kBounceTerminate;     // loop condition, ref: Main.cpp:404
    return result;
}

// ---- brute-force integrator: TracePath (ref: Source/Main.cpp:581-689) ----------------------------------------------------
// The reference recurses; every level applies one multiplicative operation to what its single child returns, innermost
// first.  Float multiplication is not associative, so the chain is recorded on the way down (one BruteLevel per bounce) and
// applied on the way back up in the reference's order, which keeps the result bit-identical to the recursion.
struct BruteLevel {
    uint32_t kind;      // 0: L = 0 + albedo*L (mirror, dielectric reflect/refract from outside)   ref: Main.cpp:618,656,672
                        // 1: same, then L *= absorption (refract out of the medium, Beer)          ref: Main.cpp:658-666
                        // 2: L = 0 + (2*pi*brdf) * (cosi*L) (uniform-hemisphere diffuse)            ref: Main.cpp:679-685
    V3 a; float cosi; V3 absorb;
};
static constexpr uint32_t kMaxBruteLevels = 32;   // max_ray_depth + 1 levels are kept in per-lane scratch

enum : uint32_t { kBruteContinue = 0u, kBruteLeaf = 1u };

// One TracePath level after IntersectScene(ray): either a leaf (returns its radiance in `leaf`) or a bounce (fills `level`,
// replaces `ray` by the child ray).  RNG draw order as in the reference: r, then Fresnel choice or the hemisphere sample (or, a rough lobe, the
// draws of ggx_sample / rough_glass_sample; a rough lobe on the wrong side of the horizon is a black leaf, as the smooth lobe's total
// internal reflection is).
template <bool COUNT, int LOBES = 0>
__device__ __forceinline__ uint32_t brute_bounce(const DevScene& sc, const DevSettings& st, Ray& ray, uint32_t& rng, uint32_t depth,
                                                 BruteLevel& level, V3& leaf, Counters& cnt)
{
    constexpr bool ROUGH_SPECULAR = HasRoughSpecular(LOBES), ROUGH_DIELECTRIC = HasRoughDielectric(LOBES);
    if (depth == 0 && st.debug_mode == 2u) {                                  // ref: Main.cpp:594-597
        leaf = bvh_depth_colour(ray);
        return kBruteLeaf;
    }
    if (ray.obj == kNoHit) { leaf = mk(0.0f); return kBruteLeaf; }            // ref: Main.cpp:600-601
    const Hit hit = get_hit<COUNT, ReadsSmoothNormals(LOBES), HonoursTransforms(LOBES)>(sc, ray, cnt);
    const Mat mat = load_material(sc, hit.mat);
    if (mat.is_light) { leaf = mat.emissive * mat.intensity; return kBruteLeaf; }   // ref: Main.cpp:606-609

    const float r = random_float(rng);                                        // ref: Main.cpp:611
    level.cosi = 0.0f; level.absorb = mk(1.0f);
    if (ROUGH_SPECULAR && r < mat.specular && mat.alpha > 0.0f) {                     // rough specular lobe: L = 0 + (albedo * G2/G1) * L
        V3 gd; float g;
        if (!ggx_sample(rng, ray.d, hit.normal, mat.alpha, gd, g)) { leaf = mk(0.0f); return kBruteLeaf; }
        ray = next_ray(hit, gd);
        level.kind = 0u; level.a = mat.albedo * g;
    } else if (r < mat.specular) {                                            // ref: Main.cpp:614-619
        ray = next_ray(hit, reflect(ray.d, hit.normal));
        level.kind = 0u; level.a = mat.albedo;
    } else if (ROUGH_DIELECTRIC && r < mat.specular + mat.refractivity && mat.alpha_t > 0.0f) {   // rough dielectric lobe
        V3 gd; float g; bool inside;
        const uint32_t kind = rough_glass_sample(rng, ray.d, hit.normal, mat.alpha_t, mat.ior, gd, g, inside);
        if (kind == kRoughGlassNone) { leaf = mk(0.0f); return kBruteLeaf; }
        level.kind = kind == kRoughGlassRefract && inside ? 1u : 0u; level.a = mat.albedo * g;
        if (level.kind == 1u) level.absorb = beer_absorption(mat, ray.t);
        ray = next_ray(hit, gd);
    } else if (r < mat.specular + mat.refractivity) {                         // ref: Main.cpp:621-675
        V3 gd; bool inside;
        const uint32_t kind = smooth_glass(mat, hit, ray, rng, gd, inside);
        if (kind == kGlassTir) { leaf = mk(0.0f); return kBruteLeaf; }        // total internal reflection: black (ref: Main.cpp:645)
        level.kind = kind == kGlassRefract && inside ? 1u : 0u; level.a = mat.albedo;
        if (level.kind == 1u) level.absorb = beer_absorption(mat, ray.t);
        ray = next_ray(hit, gd);
    } else {                                                                  // ref: Main.cpp:677-686
        const V3 dd = uniform_hemisphere_sample(rng, hit.normal);
        level.kind = 2u;
        level.cosi = dot(dd, hit.normal);
        level.a = (2.0f * kPi) * (mat.albedo * kInvPi);
        ray = next_ray(hit, dd);
    }
    return kBruteContinue;
}

// the parent's operation on its child's radiance L
__device__ __forceinline__ V3 brute_apply(const BruteLevel& lv, V3 L)
{
    if (lv.kind == 2u) {
        const V3 irr = mk(L.x * lv.cosi, L.y * lv.cosi, L.z * lv.cosi);
        return mk(0.0f) + lv.a * irr;
    }
    V3 out = mk(0.0f) + lv.a * L;
    if (lv.kind == 1u) out = out * lv.absorb;
    return out;
}

// a BruteLevel as the two float4 the kernels that keep the chain in HBM store per level
__device__ __forceinline__ void brute_pack(const BruteLevel& lv, float4& r0, float4& r1)
{
    r0.x = __uint_as_float(lv.kind); r0.y = lv.a.x; r0.z = lv.a.y; r0.w = lv.a.z;
    r1.x = lv.cosi; r1.y = lv.absorb.x; r1.z = lv.absorb.y; r1.w = lv.absorb.z;
}
__device__ __forceinline__ BruteLevel brute_unpack(float4 r0, float4 r1)
{
    BruteLevel b;
    b.kind = __float_as_uint(r0.x); b.a = mk(r0.y, r0.z, r0.w); b.cosi = r1.x; b.absorb = mk(r1.y, r1.z, r1.w);
    return b;
}

// One TracePath level of a path at `depth` on the hit of `ray` (ref: Main.cpp:581-689), for every render kernel: the bounce's operation is
// recorded with store(depth, level) and the path goes on with the child ray (returns false; depth is one more), or the path is finished
// (returns true): the recorded chain, load(k) for k = depth-1 .. 0, is folded over the leaf's radiance, innermost level first, into L.
// Where the chain lives is the caller's business.  When the depth cut-off fires -- the child returns black before tracing (ref:
// Main.cpp:589-590) -- the level just made is applied from registers instead of being stored and loaded back: brute_apply(level, 0) is what
// the fold's first step would compute.
template <bool COUNT, int LOBES, class Store, class Load>
__device__ __forceinline__ bool brute_level(const DevScene& sc, const DevSettings& st, Ray& ray, uint32_t& rng, uint32_t& depth, Store store, Load load,
                                            V3& L, Counters& cnt)
{
    BruteLevel lv;
    L = mk(0.0f);
    uint32_t stored = depth;                                                  // levels 0 .. stored-1 are recorded
    if (brute_bounce<COUNT, LOBES>(sc, st, ray, rng, depth, lv, L, cnt) != kBruteLeaf) {
        depth++;
        if ((int32_t)depth <= st.max_ray_depth) { store(stored, lv); return false; }
        L = brute_apply(lv, mk(0.0f));
    }
    while (stored-- > 0u) L = brute_apply(load(stored), L);
    return true;
}

// final colour of a finished path (ray-depth debug view, ref: Main.cpp:575-576)
__device__ __forceinline__ V3 final_energy(const DevSettings& st, const PathState& ps)
{
    if (st.debug_mode == 1u) return lerp(mk(0.0f, 1.0f, 0.0f), mk(1.0f, 0.0f, 0.0f), (float)ps.depth / (float)st.max_ray_depth);
    return ps.energy;
}

}  // namespace dev
}  // namespace cgpt
