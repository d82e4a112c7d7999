// host_shade_ris.hip -- shade_bounce's NEE block (shade_device.hpp) compiled for the HOST as it stands (float32): every
// __device__ function of the two device headers becomes __host__ __device__, and main() runs one bounce per sample on the floor of
// tests/ris_ref.py's R1 (a plane under eight sphere lights, one of them 100 times as bright) at three points, M candidates, N samples,
// against the closed form a / pi sum_k pi r_k^2 cos(theta_k) / D_k^2 L_k in double.  No GPU needed.
//   hipcc -O2 -std=c++17 -ffp-contract=off --offload-host-only -Iinclude -Icpugpupathtracing_amd/csrc/host -Icpugpupathtracing_amd/csrc/device
//         scripts/host_shade_ris.hip -o host_shade_ris && for M in 1 2 8 32; do ./host_shade_ris $M 2000000; done; ./host_shade_ris 8 2000000 later     (profiles/r14/host_shade_ris.txt)
// Prints per point and channel: mean, closed form, (mean - closed form) / standard error.  Exit status 1 if any is beyond 2.5.
#include <hip/hip_runtime.h>
#include <cstring>
static inline __host__ unsigned int __float_as_uint(float x) { unsigned int u; std::memcpy(&u, &x, 4); return u; }
static inline __host__ float __uint_as_float(unsigned int u) { float x; std::memcpy(&x, &u, 4); return x; }
#undef __device__
#define __device__ __host__ __attribute__((device))
#include "shade_device.hpp"
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <cmath>
using namespace cgpt; using namespace cgpt::dev;
int main(int argc, char** argv)
{
    const uint32_t M = argc > 1 ? atoi(argv[1]) : 8;
    const long N = argc > 2 ? atol(argv[2]) : 2000000;
    const bool later = argc > 3;                                               // a later bounce: throughput (0.8, 0.9, 0.7), floor specular 0.4 (diffuse weight 0.6)
    const float tp[3] = { later ? 0.8f : 1.0f, later ? 0.9f : 1.0f, later ? 0.7f : 1.0f }, spec = later ? 0.4f : 0.0f;
    // R1: plane floor (object 0, material 0) under eight sphere lights (objects 1..8, materials 1..8)
    std::vector<DevObject> objs(9, DevObject{}); std::vector<float4> mats(4 * 9); std::vector<uint32_t> lights;
    objs[0].kind = 2; objs[0].mat_index = 0; objs[0].plane_normal[1] = 1.0f;
    mats[0] = make_float4(0.9f, 0.7f, 0.5f, spec); mats[1] = make_float4(0, 0, 0, 0); mats[2] = make_float4(1, 0, 0, 0); mats[3] = make_float4(0, 0, 0, 0);
    const float cols[3][3] = { { 1.0f, 0.6f, 0.3f }, { 0.3f, 0.6f, 1.0f }, { 0.6f, 1.0f, 0.5f } };
    for (int k = 0; k < 8; ++k) {
        const double phi = (k + 0.37) * M_PI / 4.0;
        DevObject& o = objs[1 + k];
        o.kind = 1; o.mat_index = 1 + k;
        o.sphere_center[0] = (float)(9.0 * cos(phi)); o.sphere_center[1] = (float)(7.0 + 0.5 * (k % 3)); o.sphere_center[2] = (float)(9.0 * sin(phi));
        o.sphere_radius = k == 2 ? 0.35f : 1.5f; o.sphere_radius_sq = o.sphere_radius * o.sphere_radius;
        float4* m = &mats[4 * (1 + k)];
        m[0] = make_float4(0, 0, 0, 0); m[1] = make_float4(0, 0, 0, 0);
        if (k == 2) m[2] = make_float4(1.0f, 1.0f, 0.9f, 0.8f); else m[2] = make_float4(1.0f, cols[k % 3][0], cols[k % 3][1], cols[k % 3][2]);
        m[3] = make_float4(k == 2 ? 100.0f : 1.0f, __uint_as_float(1u), 0, 0);
        lights.push_back(1 + k);
    }
    DevScene sc{}; sc.objects = objs.data(); sc.materials = mats.data(); sc.lights = lights.data(); sc.n_objects = 9; sc.n_lights = 8;
    DevSettings st{}; st.max_ray_depth = 0; st.nee = M; st.cosine = 1; st.rr = 0; st.render_mode = 2; st.debug_mode = 0;
    const float pts[3][3] = { { 0.0f, 0.0f, 0.0f }, { -2.5f, 0.0f, -1.5f }, { 2.0f, 0.0f, 1.0f } };
    int bad = 0;
    for (int p = 0; p < 3; ++p) {
        double sum[3] = { 0, 0, 0 }, sq[3] = { 0, 0, 0 };
        for (long i = 0; i < N; ++i) {
            Ray ray = make_ray(mk(pts[p][0], 2.0f, pts[p][2]), mk(0.0f, -1.0f, 0.0f), 2.0f); ray.obj = 0;
            PathState ps; ps.throughput = mk(tp[0], tp[1], tp[2]); ps.energy = mk(0.0f); ps.rng = pcg_seed((uint32_t)i, (uint32_t)p, 12345u + M); ps.depth = 0; ps.is_specular = false;
            Ray shadow = make_ray(mk(0.0f), mk(0.0f), 0.0f); V3 pending = mk(0.0f); Counters cnt = { 0, 0, 0, 0, 0 };
            uint32_t f = M > 1 ? shade_bounce<false, 0, true>(sc, st, ray, ps, shadow, pending, cnt) : shade_bounce<false, 0, false>(sc, st, ray, ps, shadow, pending, cnt);
            if (f & kBounceShadow) { const double v[3] = { pending.x, pending.y, pending.z }; for (int c = 0; c < 3; ++c) { sum[c] += v[c]; sq[c] += v[c] * v[c]; } }
        }
        double want[3] = { 0, 0, 0 };                                          // closed form in double
        for (int k = 0; k < 8; ++k) {
            const DevObject& o = objs[1 + k]; const float4* m = &mats[4 * (1 + k)];
            const double dx = o.sphere_center[0] - pts[p][0], dy = o.sphere_center[1], dz = o.sphere_center[2] - pts[p][2];
            const double D2 = dx * dx + dy * dy + dz * dz, E = M_PI * (double)o.sphere_radius * o.sphere_radius * dy / sqrt(D2) / D2;
            const double L[3] = { (double)m[2].y * m[3].x, (double)m[2].z * m[3].x, (double)m[2].w * m[3].x };
            const double a[3] = { mats[0].x, mats[0].y, mats[0].z };
            for (int c = 0; c < 3; ++c) want[c] += E * L[c] * a[c] / M_PI * (double)tp[c] * (1.0 - (double)spec);
        }
        printf("M %2u%s  point (%g, %g)", M, later ? " later bounce" : "", pts[p][0], pts[p][2]);
        for (int c = 0; c < 3; ++c) {
            const double m = sum[c] / N, se = sqrt((sq[c] / N - m * m) / N), off = (m - want[c]) / se;
            printf("   %.7f vs %.7f: %+.2f se", m, want[c], off);
            if (fabs(off) > 2.5) bad = 1;
        }
        printf("\n");
    }
    return bad;
}
