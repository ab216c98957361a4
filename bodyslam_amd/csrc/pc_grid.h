// The uniform grid of the cloud-to-cloud distances and the walk over it, shared by the query (pointcloud.hip, bs_pc_query_grid), the
// ICP step (icp.hip, bs_icp_step), the k-nearest-neighbour query (knn.hip, bs_pc_query_knn) and the radius search (radius.hip,
// bs_pc_radius_*, bs_pc_dbscan_*): one copy of the cell function, the candidate test, the 16-byte record load, the conservative bound
// and the radius cut-off, so the kernels cannot drift apart.  The arithmetic and the derivation of the bound are at the top of pointcloud.hip.
#pragma once
#include <math.h>

#include "common.h"

namespace bs {

constexpr int PC_NONE = 0x7fffffff;                 // "no neighbour yet": above every index

__device__ __forceinline__ bool pc_finite(float v) { return fabsf(v) < INFINITY; }          // false for NaN

struct PcGrid {
    float lo[3], hi[3], h;
    int32_t n[3];
};

__device__ __forceinline__ int pc_cell(float x, float lo, float h, int n) {
    float t = floorf(__fdiv_rn(x - lo, h));
    t = fminf(fmaxf(t, 0.0f), (float)(n - 1));
    return (int)t;
}

__device__ __forceinline__ void pc_candidate(const f32x4 t, float sx, float sy, float sz, float& best, int32_t& bi) {
    const float dx = sx - t[0], dy = sy - t[1], dz = sz - t[2];
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    const int32_t id = __float_as_int(t[3]);
    if (d2 < best || (d2 == best && id < bi)) { best = d2; bi = id; }
}

// The k = 1 sink of the walk below: the minimum of (d2, original index).
struct PcMinSink {
    float sx, sy, sz, best;
    int32_t bi;
    __device__ __forceinline__ void add(const f32x4 t) { pc_candidate(t, sx, sy, sz, best, bi); }
    __device__ __forceinline__ bool bounded(float lb2) const { return best < lb2; }      // nothing unvisited can change the result
};

// The Chebyshev shells r = 0, 1, 2, ... of cells around the (clamped) cell of the finite source (sx, sy, sz), ONE copy for every kernel
// that searches the grid: each record goes to sink.add(record); after a shell the search is complete when sink.bounded(lb * lb) -- what
// the sink keeps is strictly below the bound on everything unvisited --, when every cell has been seen, or when the shell covers
// max_distance: true.  false: the source was still searching after shell `shell_cap` (the caller finishes it some other way).
// Rec: what a cell lists -- the 16-byte point records here, int32 triangle references in mesh_scene.hip (a triangle is listed in every cell its
// padded box overlaps, so after shell r the box of an unseen triangle is disjoint from the visited block and the bound holds for all its points).
template <typename Sink, typename Rec = f32x4>
__device__ __forceinline__ bool pc_walk(const Rec* __restrict__ records, const int32_t* __restrict__ cell_start, const PcGrid& g, float sx,
                                        float sy, float sz, float max_distance, int32_t shell_cap, Sink& sink) {
    const int nx = g.n[0], ny = g.n[1], nz = g.n[2];
    const int cx = pc_cell(sx, g.lo[0], g.h, nx), cy = pc_cell(sy, g.lo[1], g.h, ny), cz = pc_cell(sz, g.lo[2], g.h, nz);
    const float slack = fmaxf(fmaxf((g.hi[0] - g.lo[0]) + fabsf(sx - g.lo[0]), (g.hi[1] - g.lo[1]) + fabsf(sy - g.lo[1])),
                              (g.hi[2] - g.lo[2]) + fabsf(sz - g.lo[2])) * 4.76837158203125e-07f;       // 2^-21
    const int r_all = max(max(max(cx, nx - 1 - cx), max(cy, ny - 1 - cy)), max(cz, nz - 1 - cz));      // after this shell: every cell seen
    for (int r = 0;; ++r) {
        const int z0 = max(cz - r, 0), z1 = min(cz + r, nz - 1), y0 = max(cy - r, 0), y1 = min(cy + r, ny - 1);
        const int x0 = max(cx - r, 0), x1 = min(cx + r, nx - 1);
        for (int z = z0; z <= z1; ++z)
            for (int y = y0; y <= y1; ++y) {
                const int row = (z * ny + y) * nx;
                // the row's records as up to two runs, and ONE place where a record meets the sink: a sink that keeps a list in registers
                // (knn.hip) is inlined once, not three times
                int32_t b0 = 0, e0 = 0, b1 = 0, e1 = 0;
                if (abs(z - cz) == r || abs(y - cy) == r) {             // a face row of the shell: its cells are one run of records
                    b0 = cell_start[row + x0];
                    e0 = cell_start[row + x1 + 1];
                } else {                                                // an inner row: the two end cells
                    if (cx - r >= 0) { b0 = cell_start[row + cx - r]; e0 = cell_start[row + cx - r + 1]; }
                    if (cx + r <= nx - 1) { b1 = cell_start[row + cx + r]; e1 = cell_start[row + cx + r + 1]; }
                }
#pragma clang loop unroll(disable)
                for (int part = 0; part < 2; ++part) {
                    const int32_t e = part ? e1 : e0;
                    for (int32_t k = part ? b1 : b0; k < e; ++k) sink.add(records[k]);
                }
            }
        if (r >= r_all) return true;
        const float lb = ((float)r * g.h - slack) * 0.99999f;
        if (lb > 0.0f && sink.bounded(lb * lb)) return true;
        if (lb * 0.9999f > max_distance) return true;
        if (r >= shell_cap) return false;
    }
}

// The k = 1 search: best = the minimum d2, bi = its original index (PC_NONE: no candidate seen).
__device__ __forceinline__ bool pc_walk_shells(const f32x4* __restrict__ records, const int32_t* __restrict__ cell_start, const PcGrid& g,
                                               float sx, float sy, float sz, float max_distance, int32_t shell_cap, float& best, int32_t& bi) {
    PcMinSink sink{sx, sy, sz, INFINITY, PC_NONE};
    const bool done = pc_walk(records, cell_start, g, sx, sy, sz, max_distance, shell_cap, sink);
    best = sink.best;
    bi = sink.bi;
    return done;
}

// The radius of the hybrid search (knn.hip) and of the radius search (radius.hip) as a cut-off on d2: the largest fp32 d2 with
// sqrtf(d2) <= radius (host arithmetic: sqrtf is correctly rounded and monotone), so d2 <= cut-off is the same predicate without a
// square root per candidate.
inline float knn_d2_cutoff(float radius) {
    if (!(radius < INFINITY)) return INFINITY;
    float c = radius * radius;
    if (!(c < INFINITY)) c = 3.402823466e+38f;
    while (c > 0.0f && sqrtf(c) > radius) c = nextafterf(c, 0.0f);
    for (;;) {
        const float up = nextafterf(c, INFINITY);
        if (!(up < INFINITY) || sqrtf(up) > radius) break;
        c = up;
    }
    return c;
}

inline bool pc_grid_ok(const PcGrid& g) {
    if (!(g.h > 0.0f) || !isfinite(g.h)) return false;
    int64_t cells = 1;
    for (int a = 0; a < 3; ++a) {
        if (g.n[a] < 1 || !isfinite(g.lo[a]) || !isfinite(g.hi[a]) || !(g.hi[a] >= g.lo[a])) return false;
        cells *= g.n[a];
        if (cells > BS_PC_MAX_CELLS) return false;
    }
    return true;
}
inline PcGrid pc_grid(const float* lo, const float* hi, float h, const int32_t* dims) {
    PcGrid g;
    for (int a = 0; a < 3; ++a) { g.lo[a] = lo[a]; g.hi[a] = hi[a]; g.n[a] = dims[a]; }
    g.h = h;
    return g;
}

}  // namespace bs
