// The triangle rule shared by the mesh scene (mesh_scene.hip: records, ray hits, sampling) and mesh clean-up (mesh_ops.hip: triangle
// geometry): one copy of the validity test, the fp32 cross product with the KEPT rule, the unit normal and the fp64 cross product and area,
// so a RaycastingScene and a TriangleMesh keep the same triangles and give the same normals bit for bit.  The statement is
// tests/_mesh_scene_ref.py; the arithmetic is at the top of mesh_scene.hip.  A vertex P is anything with P[0], P[1], P[2] as fp32: an f32x4
// record or a float[3].  No contraction (the build has -ffp-contract=off), every division and square root correctly rounded.
#pragma once
#include <math.h>

#include "common.h"
#include "pc_grid.h"

namespace bs {

// the three indices of triangle t; true when it is VALID: they lie in [0, V) and are pairwise distinct
__device__ __forceinline__ bool tri_indices(const int32_t* __restrict__ triangles, int64_t t, int64_t n_vertices, int32_t (&v)[3]) {
    v[0] = triangles[3 * t]; v[1] = triangles[3 * t + 1]; v[2] = triangles[3 * t + 2];
    return v[0] >= 0 && v[0] < n_vertices && v[1] >= 0 && v[1] < n_vertices && v[2] >= 0 && v[2] < n_vertices && v[0] != v[1] && v[1] != v[2] &&
           v[2] != v[0];
}

template <class P>
__device__ __forceinline__ bool tri_finite3(const P p) { return pc_finite(p[0]) && pc_finite(p[1]) && pc_finite(p[2]); }

// n = (b - a) x (c - a) in fp32; true when the triangle is KEPT: the nine coordinates and n are finite and n != 0
template <class P>
__device__ __forceinline__ bool tri_cross(const P a, const P b, const P c, float (&n)[3]) {
    const float e1x = b[0] - a[0], e1y = b[1] - a[1], e1z = b[2] - a[2], e2x = c[0] - a[0], e2y = c[1] - a[1], e2z = c[2] - a[2];
    n[0] = e1y * e2z - e1z * e2y;
    n[1] = e1z * e2x - e1x * e2z;
    n[2] = e1x * e2y - e1y * e2x;
    return tri_finite3(a) && tri_finite3(b) && tri_finite3(c) && pc_finite(n[0]) && pc_finite(n[1]) && pc_finite(n[2]) &&
           (n[0] != 0.0f || n[1] != 0.0f || n[2] != 0.0f);
}

// the unit normal of a kept triangle from its cross product: m = max |n_a|, s = n / m, u = s / |s|
__device__ __forceinline__ void tri_unit(const float (&n)[3], float (&u)[3]) {
    const float m = fmaxf(fmaxf(fabsf(n[0]), fabsf(n[1])), fabsf(n[2]));
    const float sx = __fdiv_rn(n[0], m), sy = __fdiv_rn(n[1], m), sz = __fdiv_rn(n[2], m);
    const float len = sqrtf((sx * sx + sy * sy) + sz * sz);
    u[0] = __fdiv_rn(sx, len); u[1] = __fdiv_rn(sy, len); u[2] = __fdiv_rn(sz, len);
}

template <class P>
__device__ __forceinline__ void tri_unit_normal(const P a, const P b, const P c, float (&u)[3]) {
    float n[3];
    tri_cross(a, b, c, n);
    tri_unit(n, u);
}

// the fp64 cross product of the fp64 differences of the fp32 vertices, and the area it gives
template <class P>
__device__ __forceinline__ void tri_cross64(const P a, const P b, const P c, double (&n)[3]) {
    const double e1x = (double)b[0] - (double)a[0], e1y = (double)b[1] - (double)a[1], e1z = (double)b[2] - (double)a[2];
    const double e2x = (double)c[0] - (double)a[0], e2y = (double)c[1] - (double)a[1], e2z = (double)c[2] - (double)a[2];
    n[0] = e1y * e2z - e1z * e2y;
    n[1] = e1z * e2x - e1x * e2z;
    n[2] = e1x * e2y - e1y * e2x;
}
__device__ __forceinline__ double tri_area64(const double (&n)[3]) { return 0.5 * sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]); }

// The cells of one axis a kept triangle is referenced from in the triangle grid (a, b, c: its three coordinates on that axis): what the
// build scatters to (mesh_scene.hip), what the counting walk takes the first cell of a run from, and what the pair search takes the first
// common cell of two triangles from (mesh_solid.hip) -- one expression, so they cannot disagree.
__device__ __forceinline__ void ms_cell_range(float a, float b, float c, float pad, float lo, float h, int n, int& c0, int& c1) {
    c0 = pc_cell(fminf(fminf(a, b), c) - pad, lo, h, n);
    c1 = pc_cell(fmaxf(fmaxf(a, b), c) + pad, lo, h, n);
}

}  // namespace bs
