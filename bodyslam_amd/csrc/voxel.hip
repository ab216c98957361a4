// Voxel down-sampling of a point cloud (bs_pc_voxel_assign, bs_pc_voxel_flags, bs_pc_voxel_accumulate, bs_pc_voxel_finish;
// include/bodyslam_hip.h): the role of Open3D's PointCloud.voxel_down_sample, which the reference calls at
// BodySLAM_not_refactored/3DM/mapping_module.py:72,156,187.  Restated from Open3D's documented meaning; parity with Open3D is UNPINNED.
// The statement is tests/_voxel_ref.py.
//
// Four launches, nothing but stream order between them:
//   assign      one thread per point: v = floor(((double) p - o) / h) per axis, key = vz << 42 | vy << 21 | vx, inserted into the open-addressing
//               table of 64-bit keys of slot_table.h (slot_insert, shared with mesh_ops.hip: linear probing from a mixed hash, atomicCAS on
//               the key), then atomicMin of the point index on the slot's `first`.  A slot goes from EMPTY to its key once and never changes again, so a relaxed load that shows a key other than
//               EMPTY is final: only an EMPTY slot needs the CAS.  `first` only decreases, so a relaxed load at or below the point's index
//               saves the atomicMin: at h = 0.05 m a voxel of the 1 mm map holds thousands of points and nearly all of them skip it.
//               The probe loop ends after `slots` probes with the status bit BS_PC_VOXEL_TABLE_FULL: a full table costs an error, never
//               a spinning wave.
//   flags       slot_table.h's flags kernel: leader[i] = first[slot_i], is_first[i] = (leader[i] == i).  The caller's inclusive scan of is_first (integer, exact) is the
//               rank: the voxel led by point j has row rank[j] - 1 -- first appearance order, whatever slot the voxel got.
//   accumulate  one thread per point adds its 3, 6 or 9 int64 terms Q and a count to its row with 64-bit integer atomics.  Integer addition
//               is associative, so any pre-summing is exact: a run of adjacent lanes with the same row (clouds from depth images and from
//               extract_pcd come in such runs) is summed in the wave by a segmented scan over shuffles, and the run's last lane issues the
//               atomics.  A wave without two equal neighbours skips the scan.
//   finish      one thread per row: the division, the single-point rule, unit_normals, the fp32 stores.
// No floating-point atomics: the sums are integers, so the result depends on neither the slot of a voxel, nor the size of the table, nor the
// order the atomics arrive in.  Every index read from memory is checked against its array before it is used.
#include <math.h>

#include "common.h"
#include "pc_grid.h"
#include "slot_table.h"

namespace bs {
namespace {

constexpr int VOXEL_THREADS = 256;
constexpr int VOXEL_ATTR_SHIFT = 30;
typedef slot_key voxel_key;

struct VoxelOrigin { double o[3]; };

__global__ void __launch_bounds__(VOXEL_THREADS) voxel_assign_kernel(const float* __restrict__ pts, int64_t n, VoxelOrigin org, double h,
                                                                     voxel_key* __restrict__ keys, int32_t* __restrict__ first, int64_t slots,
                                                                     int32_t* __restrict__ slot_of_point, int32_t* __restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * VOXEL_THREADS + threadIdx.x;
    if (i >= n) return;
    const float x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    int32_t found = -1;
    if (pc_finite(x) && pc_finite(y) && pc_finite(z)) {
        const double limit = (double)(1 << BS_PC_VOXEL_AXIS_BITS);
        const double vx = floor(((double)x - org.o[0]) / h), vy = floor(((double)y - org.o[1]) / h), vz = floor(((double)z - org.o[2]) / h);
        if (vx >= 0.0 && vx < limit && vy >= 0.0 && vy < limit && vz >= 0.0 && vz < limit) {
            found = slot_insert(keys, slots, ((voxel_key)vz << 42) | ((voxel_key)vy << 21) | (voxel_key)vx);
            if (found < 0) {
                atomicOr(status, BS_PC_VOXEL_TABLE_FULL);
            } else if (__hip_atomic_load(&first[found], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > (int32_t)i) {
                // `first` only ever decreases: a value at or below i, however old, means the minimum is not i's to lower
                atomicMin(&first[found], (int32_t)i);
            }
        } else {
            atomicOr(status, BS_PC_VOXEL_OUT_OF_RANGE);
        }
    }
    slot_of_point[i] = found;
}

// Q of an attribute component; false when it is not finite with |a| <= 2
__device__ __forceinline__ bool voxel_attr_q(float a, long long& q) {
    const bool ok = fabsf(a) <= 2.0f;                                                   // false for NaN
    q = ok ? (long long)rint(ldexp((double)a, VOXEL_ATTR_SHIFT)) : 0ll;
    return ok;
}

template <int T>
__global__ void __launch_bounds__(VOXEL_THREADS) voxel_accumulate_kernel(const float* __restrict__ pts, const float* __restrict__ colors,
                                                                         const float* __restrict__ normals, int64_t n, VoxelOrigin org, int shift,
                                                                         const int32_t* __restrict__ leader, const int32_t* __restrict__ rank,
                                                                         int64_t m, voxel_key* __restrict__ sums, int32_t* __restrict__ counts,
                                                                         int32_t* __restrict__ first_index, int32_t* __restrict__ row_of_point,
                                                                         int32_t* __restrict__ status) {
    // (no early return: every lane of the wave takes part in the shuffles below; the block is a whole number of waves)
    const int64_t i = (int64_t)blockIdx.x * VOXEL_THREADS + threadIdx.x;
    int32_t row = -1;
    long long q[T];
#pragma unroll
    for (int t = 0; t < T; ++t) q[t] = 0;
    if (i < n) {
        const int32_t ld = leader[i];
        if (ld >= 0 && ld < n) {
            const int32_t r = rank[ld] - 1;
            if (r >= 0 && r < m) row = r;
        }
        if (row >= 0) {
#pragma unroll
            for (int a = 0; a < 3; ++a) q[a] = (long long)rint(ldexp((double)pts[3 * i + a] - org.o[a], shift));
            bool ok = true;
            if (T >= 6) {
                const float* __restrict__ attr = colors ? colors : normals;
#pragma unroll
                for (int a = 0; a < 3; ++a) ok &= voxel_attr_q(attr[3 * i + a], q[3 + a]);
            }
            if (T == 9) {
#pragma unroll
                for (int a = 0; a < 3; ++a) ok &= voxel_attr_q(normals[3 * i + a], q[6 + a]);
            }
            if (!ok) atomicOr(status, BS_PC_VOXEL_BAD_ATTRIBUTE);
            if (ld == (int32_t)i) first_index[row] = (int32_t)i;
        }
        row_of_point[i] = row;
    }
    int32_t cnt = 1;
    const int lane = threadIdx.x & 63;
    const int32_t before = __shfl_up(row, 1);
    const unsigned long long heads = __ballot(lane == 0 || before != row);               // bit l: lane l begins a run of equal rows
    if (heads != ~0ull) {
        const int start = 63 - __builtin_clzll(heads & (~0ull >> (63 - lane)));          // the run's first lane (bit 0 is always set)
#pragma unroll
        for (int d = 1; d < 64; d *= 2) {
            const bool take = lane - d >= start;
            const int32_t c = __shfl_up(cnt, d);
            cnt += take ? c : 0;
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const long long v = __shfl_up(q[t], d);
                q[t] += take ? v : 0ll;
            }
        }
    }
    const bool last = lane == 63 || ((heads >> (lane + 1)) & 1ull);                       // the run's last lane holds its sums
    if (last && row >= 0) {
        atomicAdd(&counts[row], cnt);
#pragma unroll
        for (int t = 0; t < T; ++t) atomicAdd(&sums[(int64_t)row * T + t], (voxel_key)q[t]);
    }
}

__global__ void __launch_bounds__(VOXEL_THREADS) voxel_finish_kernel(const float* __restrict__ pts, const float* __restrict__ colors,
                                                                     const float* __restrict__ normals, int64_t n,
                                                                     const voxel_key* __restrict__ sums, const int32_t* __restrict__ counts,
                                                                     const int32_t* __restrict__ first_index, int64_t m, int terms,
                                                                     VoxelOrigin org, int shift, int unit_normals, float* __restrict__ out_points,
                                                                     float* __restrict__ out_colors, float* __restrict__ out_normals) {
    const int64_t r = (int64_t)blockIdx.x * VOXEL_THREADS + threadIdx.x;
    if (r >= m) return;
    const int32_t count = counts[r];
    const int64_t f = first_index[r];
    const bool single = count == 1 && f >= 0 && f < n;
    const double c = (double)count;
    const voxel_key* __restrict__ S = sums + r * terms;
#pragma unroll
    for (int a = 0; a < 3; ++a)
        out_points[3 * r + a] = single ? pts[3 * f + a] : (float)(org.o[a] + ldexp((double)(long long)S[a] / c, -shift));
    int at = 3;
    if (colors) {
#pragma unroll
        for (int a = 0; a < 3; ++a)
            out_colors[3 * r + a] = single ? colors[3 * f + a] : (float)ldexp((double)(long long)S[at + a] / c, -VOXEL_ATTR_SHIFT);
        at += 3;
    }
    if (normals) {
        double d[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) d[a] = ldexp((double)(long long)S[at + a] / c, -VOXEL_ATTR_SHIFT);
        if (unit_normals) {
            const double len = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
#pragma unroll
            for (int a = 0; a < 3; ++a) out_normals[3 * r + a] = len > 0.0 ? (float)(d[a] / len) : 0.0f;
        } else {
#pragma unroll
            for (int a = 0; a < 3; ++a) out_normals[3 * r + a] = single ? normals[3 * f + a] : (float)d[a];
        }
    }
}

bool voxel_origin(const double* origin, VoxelOrigin& org) {
    for (int a = 0; a < 3; ++a) {
        if (!isfinite(origin[a])) return false;
        org.o[a] = origin[a];
    }
    return true;
}

}  // namespace
}  // namespace bs

extern "C" int bs_pc_voxel_assign(const float* points, int64_t n, const double* origin, double voxel_size, void* keys, int32_t* first, int64_t slots,
                                  int32_t* slot_of_point, int32_t* status, void* stream) {
    using namespace bs;
    if (!initialized()) { set_error("bs_pc_voxel_assign: call bs_init first"); return BS_ERR_NOT_INIT; }
    BS_REQUIRE(points && origin && keys && first && slot_of_point && status, "bs_pc_voxel_assign: null pointer");
    BS_REQUIRE(n >= 1 && n < ((int64_t)1 << 31), "bs_pc_voxel_assign: n = %lld (1 <= n < 2^31)", (long long)n);
    BS_REQUIRE(slots > n && slots <= ((int64_t)1 << 31) && (slots & (slots - 1)) == 0,
               "bs_pc_voxel_assign: slots = %lld (a power of two, n < slots <= 2^31)", (long long)slots);
    BS_REQUIRE(voxel_size > 0.0 && isfinite(voxel_size), "bs_pc_voxel_assign: voxel size %g", voxel_size);
    BS_REQUIRE(((uintptr_t)keys & 7) == 0, "bs_pc_voxel_assign: keys must be 8-byte aligned");
    VoxelOrigin org;
    BS_REQUIRE(voxel_origin(origin, org), "bs_pc_voxel_assign: the origin is not finite");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(voxel_assign_kernel, dim3((unsigned)cdiv64(n, VOXEL_THREADS)), dim3(VOXEL_THREADS), 0, st, points, n, org, voxel_size,
                       static_cast<voxel_key*>(keys), first, slots, slot_of_point, status);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_pc_voxel_flags(const int32_t* slot_of_point, const int32_t* first, int64_t slots, int64_t n, int32_t* leader, int32_t* is_first,
                                 void* stream) {
    using namespace bs;
    if (!initialized()) { set_error("bs_pc_voxel_flags: call bs_init first"); return BS_ERR_NOT_INIT; }
    BS_REQUIRE(slot_of_point && first && leader && is_first, "bs_pc_voxel_flags: null pointer");
    BS_REQUIRE(n >= 1 && n < ((int64_t)1 << 31) && slots >= 1, "bs_pc_voxel_flags: n = %lld, slots = %lld", (long long)n, (long long)slots);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    slot_flags_launch(slot_of_point, first, slots, n, leader, is_first, st);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_pc_voxel_accumulate(const float* points, const float* colors, const float* normals, int64_t n, const double* origin, int32_t shift,
                                      const int32_t* leader, const int32_t* rank, int64_t m, void* sums, int32_t* counts, int32_t* first_index,
                                      int32_t* row_of_point, int32_t* status, void* stream) {
    using namespace bs;
    if (!initialized()) { set_error("bs_pc_voxel_accumulate: call bs_init first"); return BS_ERR_NOT_INIT; }
    BS_REQUIRE(points && origin && leader && rank && sums && counts && first_index && row_of_point && status, "bs_pc_voxel_accumulate: null pointer");
    BS_REQUIRE(n >= 1 && n < ((int64_t)1 << 31) && m >= 1 && m <= n, "bs_pc_voxel_accumulate: n = %lld, m = %lld (1 <= m <= n < 2^31)", (long long)n,
               (long long)m);
    BS_REQUIRE(shift > -2048 && shift < 2048, "bs_pc_voxel_accumulate: shift %d", shift);
    BS_REQUIRE(((uintptr_t)sums & 7) == 0, "bs_pc_voxel_accumulate: sums must be 8-byte aligned");
    VoxelOrigin org;
    BS_REQUIRE(voxel_origin(origin, org), "bs_pc_voxel_accumulate: the origin is not finite");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)cdiv64(n, VOXEL_THREADS)), thr(VOXEL_THREADS);
    voxel_key* S = static_cast<voxel_key*>(sums);
#define VOXEL_ACCUMULATE(T) \
    hipLaunchKernelGGL((voxel_accumulate_kernel<T>), grid, thr, 0, st, points, colors, normals, n, org, (int)shift, leader, rank, m, S, counts, \
                       first_index, row_of_point, status)
    if (colors && normals) VOXEL_ACCUMULATE(9);
    else if (colors || normals) VOXEL_ACCUMULATE(6);
    else VOXEL_ACCUMULATE(3);
#undef VOXEL_ACCUMULATE
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_pc_voxel_finish(const float* points, const float* colors, const float* normals, int64_t n, const void* sums, const int32_t* counts,
                                  const int32_t* first_index, int64_t m, const double* origin, int32_t shift, int32_t unit_normals, float* out_points,
                                  float* out_colors, float* out_normals, void* stream) {
    using namespace bs;
    if (!initialized()) { set_error("bs_pc_voxel_finish: call bs_init first"); return BS_ERR_NOT_INIT; }
    BS_REQUIRE(points && origin && sums && counts && first_index && out_points, "bs_pc_voxel_finish: null pointer");
    BS_REQUIRE((colors == nullptr) == (out_colors == nullptr) && (normals == nullptr) == (out_normals == nullptr),
               "bs_pc_voxel_finish: an attribute needs its input and its output");
    BS_REQUIRE(n >= 1 && n < ((int64_t)1 << 31) && m >= 1 && m <= n, "bs_pc_voxel_finish: n = %lld, m = %lld (1 <= m <= n < 2^31)", (long long)n,
               (long long)m);
    BS_REQUIRE(shift > -2048 && shift < 2048, "bs_pc_voxel_finish: shift %d", shift);
    VoxelOrigin org;
    BS_REQUIRE(voxel_origin(origin, org), "bs_pc_voxel_finish: the origin is not finite");
    const int terms = 3 + (colors ? 3 : 0) + (normals ? 3 : 0);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(voxel_finish_kernel, dim3((unsigned)cdiv64(m, VOXEL_THREADS)), dim3(VOXEL_THREADS), 0, st, points, colors, normals, n,
                       static_cast<const voxel_key*>(sums), counts, first_index, m, terms, org, (int)shift, (int)(unit_normals != 0), out_points,
                       out_colors, out_normals);
    BS_CHECK_LAUNCH();
    return BS_OK;
}
