// Consistent orientation of the normals of a cloud along the minimum spanning tree of its k-NN graph (bs_pc_orient_*;
// include/bodyslam_hip.h): the role of Open3D's PointCloud.orient_normals_consistent_tangent_plane (Hoppe et al. 1992).  Restated from
// Open3D's documented meaning; parity with Open3D is UNPINNED, and no Delaunay edges are added: a disconnected k-NN graph gives several
// trees, each oriented on its own.  The statement is tests/_orient_ref.py, DESIGN section 3.24 the argument.
//
// The graph is the k-NN lists as they lie (bs_pc_query_knn of the cloud on itself): slot t = i k + c holds j = index[i][c], and the
// undirected edge {i, j} exists when it lies in either row and both ends are VALID (finite coordinates, a finite normal that is not all
// zero).  In fp64 without contraction d = (ax bx + ay by) + az bz on the fp32 normals, w = fl32(max(1 - |d|, 0)), the sign link is
// s = (d < 0).  Edges are ordered by (the bits of w, min(i, j), max(i, j)): a total order, so the minimum spanning forest is unique --
// on a plane every weight is exactly 0 and the indices alone decide.  Boruvka's rounds on that order:
//   edges       once: the 64-bit key w_bits << 32 | min(i, j) of every slot, ~0 for a slot that is no edge, and valid [n]
//   clear       best [n] = ~0, best_hi [n] = 0x7fffffff
//   select      every crossing slot -- its two ends have different roots -- offers its key to best[] of both roots by 64-bit atomicMin and
//               sets `crossing`.  A single key cannot hold w and both indices, hence
//   select_hi   the crossing slots whose key equals their root's best offer max(i, j) to best_hi[] by 32-bit atomicMin
//   hook        every root with an edge hooks (lo, hi, s) through union_parity.h; s is computed again from the two normals.  The edge is
//               its component's lightest outgoing edge and so in the unique forest whether or not the atomicMin wins: a hook that loses
//               to a smaller root is selected again in the next round
//   compress    word[x] = root << 1 | parity to the root
// until a round finds no crossing slot.  Then
//   seed        per tree the valid point of largest fp32 z (-0 counts as +0), ties to the lowest index: one 64-bit key per root,
//               (the complement of the ordered bits of z) << 32 | index, by atomicMin -- the mirror image of an atomicMax of (ordered z,
//               complemented index), so that one merging offer serves both selections
//   flip        the seed is flipped when (nx dx + ny dy) + nz dz < 0 in fp64; flip(x) = the seed's flip xor the parity of the tree path
//               from x to the seed = seed flip ^ parity(x -> root) ^ parity(seed -> root).  A flipped normal has its three sign bits
//               toggled; every other row, the invalid ones included, is copied bit for bit.
// The offers (or_offer): an offer is dropped when the slot already holds a key that is no larger -- the slots only decrease, so a stale read
// errs on the safe side --, and the lanes of a wave that offer to the same root are merged into one atomic by the ballot loop of
// mesh_ops.hip's cc_clusters_kernel with a minimum over the wave, for at most OR_MERGE_TURNS distinct roots; the lanes left after that
// issue their own.  After the first rounds most slots are internal and the crossing ones concentrate on a few roots.  What the merge saves
// (profiles/orient_merge_ab.txt: the 254 991-point cloud of the 256-frame map, three builds in one call, MI355X): with OR_MERGE_TURNS = 0
// -- the stale-read filter alone, every remaining lane its own atomic -- the select launches of a call take 1.08 ms instead of 0.73 ms at
// k = 10 and 4.41 ms instead of 2.46 ms at k = 30, and the seed launch, where nearly every lane of a wave offers to the one root, 1.78 ms
// instead of 0.04 ms: the whole call 5.6 ms instead of 2.6 ms and 9.8 ms instead of 5.5 ms.  With 64 turns (merge everything) the times are
// those of 8 within the noise.
// Integer atomics only: the minimum of a set does not depend on the order of arrival, so the forest, the parities and the seeds are the same
// in every run.  No LDS; every index read from memory is checked against its array before it is used.
#include <math.h>

#include "common.h"
#include "pc_grid.h"
#include "union_parity.h"

namespace bs {
namespace {

constexpr int OR_THREADS = 256;
constexpr int OR_MERGE_TURNS = 8;
typedef unsigned long long or_key;
constexpr or_key OR_NONE = ~0ull;
constexpr int32_t OR_NO_HI = 0x7fffffff;

__device__ __forceinline__ bool or_valid(const float* __restrict__ points, const float* __restrict__ normals, int64_t i) {
    const float nx = normals[3 * i], ny = normals[3 * i + 1], nz = normals[3 * i + 2];
    return pc_finite(points[3 * i]) && pc_finite(points[3 * i + 1]) && pc_finite(points[3 * i + 2]) && pc_finite(nx) && pc_finite(ny) &&
           pc_finite(nz) && (nx != 0.0f || ny != 0.0f || nz != 0.0f);
}

__device__ __forceinline__ double or_dot(const float* __restrict__ normals, int64_t a, int64_t b) {
    return ((double)normals[3 * a] * (double)normals[3 * b] + (double)normals[3 * a + 1] * (double)normals[3 * b + 1]) +
           (double)normals[3 * a + 2] * (double)normals[3 * b + 2];
}

// min into slot[r] for every lane with `active`; every lane of the wave calls this (the ballots)
__device__ __forceinline__ void or_offer(or_key* slot, uint32_t r, bool active, or_key key) {
    if (active && __hip_atomic_load(&slot[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= key) active = false;
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(active);
    for (int turn = 0; turn < OR_MERGE_TURNS && todo; ++turn) {
        const int first = __ffsll((long long)todo) - 1;
        const uint32_t rf = __shfl(r, first);
        const bool mine = active && r == rf;
        or_key m = mine ? key : OR_NONE;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const or_key other = __shfl_xor(m, d);
            m = other < m ? other : m;
        }
        if (lane == first) atomicMin(&slot[rf], m);
        todo &= ~__ballot(mine);
        if (mine) active = false;
    }
    if (active) atomicMin(&slot[r], key);
}

__global__ void __launch_bounds__(OR_THREADS) pc_orient_edges_kernel(const float* __restrict__ points, const float* __restrict__ normals, int64_t n,
                                                                  const int32_t* __restrict__ index, const int32_t* __restrict__ count, int k,
                                                                  or_key* __restrict__ keys, int32_t* __restrict__ valid) {
    const int64_t t = (int64_t)blockIdx.x * OR_THREADS + threadIdx.x;
    if (t >= n * k) return;
    const int64_t i = t / k;
    const int c = (int)(t - i * k);
    const bool ok = or_valid(points, normals, i);
    if (c == 0) valid[i] = ok ? 1 : 0;
    or_key key = OR_NONE;
    if (ok && c < count[i]) {
        const int64_t j = index[t];
        if (j >= 0 && j < n && j != i && or_valid(points, normals, j)) {
            const double d = or_dot(normals, i, j);
            const float w = (float)fmax(1.0 - fabs(d), 0.0);
            key = ((or_key)__float_as_uint(w) << 32) | (or_key)(uint32_t)(i < j ? i : j);
        }
    }
    keys[t] = key;
}

__global__ void __launch_bounds__(OR_THREADS) pc_orient_clear_kernel(or_key* __restrict__ best, int32_t* __restrict__ best_hi, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * OR_THREADS + threadIdx.x;
    if (i >= n) return;
    best[i] = OR_NONE;
    if (best_hi) best_hi[i] = OR_NO_HI;
}

// the two roots of a slot that is an edge; false for a slot that is none or whose ends share a root
__device__ __forceinline__ bool or_crossing(const or_key* __restrict__ keys, const int32_t* __restrict__ index, const uint32_t* word, int64_t n, int k,
                                            int64_t t, or_key& key, uint32_t& ri, uint32_t& rj, int32_t& hi) {
    if (t >= n * k) return false;
    key = keys[t];
    if (key == OR_NONE) return false;
    const int64_t i = t / k, j = index[t];
    if (j < 0 || j >= n) return false;
    uint32_t unused;
    ri = up_root(word, (uint32_t)i, n, unused);
    rj = up_root(word, (uint32_t)j, n, unused);
    hi = (int32_t)(i > j ? i : j);
    return ri != rj;
}

__global__ void __launch_bounds__(OR_THREADS) pc_orient_select_kernel(const or_key* __restrict__ keys, const int32_t* __restrict__ index,
                                                                   const uint32_t* word, int64_t n, int k, or_key* best,
                                                                   int32_t* __restrict__ crossing) {
    // (no early return: every lane of the wave takes part in the ballots; the block is a whole number of waves)
    const int64_t t = (int64_t)blockIdx.x * OR_THREADS + threadIdx.x;
    or_key key = OR_NONE;
    uint32_t ri = 0, rj = 0;
    int32_t hi;
    const bool cross = or_crossing(keys, index, word, n, k, t, key, ri, rj, hi);
    if (__ballot(cross) == 0) return;                                    // (the whole wave)
    if ((threadIdx.x & 63) == __ffsll((long long)__ballot(cross)) - 1) *crossing = 1;      // (every writer stores the same value)
    or_offer(best, ri, cross, key);
    or_offer(best, rj, cross, key);
}

__global__ void __launch_bounds__(OR_THREADS) pc_orient_select_hi_kernel(const or_key* __restrict__ keys, const int32_t* __restrict__ index,
                                                                      const uint32_t* word, int64_t n, int k, const or_key* __restrict__ best,
                                                                      int32_t* best_hi) {
    const int64_t t = (int64_t)blockIdx.x * OR_THREADS + threadIdx.x;
    or_key key;
    uint32_t ri, rj;
    int32_t hi;
    if (!or_crossing(keys, index, word, n, k, t, key, ri, rj, hi)) return;
    if (best[ri] == key && __hip_atomic_load(&best_hi[ri], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > hi) atomicMin(&best_hi[ri], hi);
    if (best[rj] == key && __hip_atomic_load(&best_hi[rj], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > hi) atomicMin(&best_hi[rj], hi);
}

__global__ void __launch_bounds__(OR_THREADS) pc_orient_hook_kernel(const float* __restrict__ normals, uint32_t* word, int64_t n,
                                                                 const or_key* __restrict__ best, const int32_t* __restrict__ best_hi) {
    const int64_t r = (int64_t)blockIdx.x * OR_THREADS + threadIdx.x;
    if (r >= n) return;
    if ((__hip_atomic_load(&word[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> 1) != (uint32_t)r) return;
    const or_key key = best[r];
    if (key == OR_NONE) return;
    const int64_t lo = (int64_t)(uint32_t)(key & 0xffffffffull), hi = best_hi[r];
    if (lo >= n || hi < 0 || hi >= n || lo == hi) return;
    up_union(word, (uint32_t)lo, (uint32_t)hi, or_dot(normals, lo, hi) < 0.0 ? 1u : 0u, n);
}

__global__ void __launch_bounds__(OR_THREADS) pc_orient_compress_kernel(uint32_t* word, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * OR_THREADS + threadIdx.x;
    if (i >= n) return;
    up_compress(word, (uint32_t)i, n);
}

__global__ void __launch_bounds__(OR_THREADS) pc_orient_seed_kernel(const float* __restrict__ points, const int32_t* __restrict__ valid,
                                                                 const uint32_t* __restrict__ word, int64_t n, or_key* seed) {
    // (no early return: the ballots)
    const int64_t i = (int64_t)blockIdx.x * OR_THREADS + threadIdx.x;
    bool active = false;
    uint32_t r = 0;
    or_key key = OR_NONE;
    if (i < n && valid[i]) {
        r = word[i] >> 1;
        if (r < n) {
            float z = points[3 * i + 2];
            if (z == 0.0f) z = 0.0f;                                     // -0 ties with +0
            const uint32_t u = __float_as_uint(z);
            const uint32_t ordered = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
            key = ((or_key)(~ordered) << 32) | (or_key)(uint32_t)i;
            active = true;
        }
    }
    or_offer(seed, r, active, key);
}

__global__ void __launch_bounds__(OR_THREADS) pc_orient_flip_kernel(const float* __restrict__ normals, const int32_t* __restrict__ valid,
                                                                 const uint32_t* __restrict__ word, int64_t n, const or_key* __restrict__ seed,
                                                                 double dx, double dy, double dz, float* __restrict__ out,
                                                                 uint8_t* __restrict__ flipped) {
    const int64_t i = (int64_t)blockIdx.x * OR_THREADS + threadIdx.x;
    if (i >= n) return;
    uint32_t flip = 0;
    if (valid[i]) {
        const uint32_t w = word[i], r = w >> 1;
        if (r < n) {
            const or_key sk = seed[r];
            const int64_t sd = (int64_t)(uint32_t)(sk & 0xffffffffull);
            if (sk != OR_NONE && sd < n) {
                const uint32_t ws = word[sd];
                if ((ws >> 1) == r) {
                    const double d = ((double)normals[3 * sd] * dx + (double)normals[3 * sd + 1] * dy) + (double)normals[3 * sd + 2] * dz;
                    flip = (d < 0.0 ? 1u : 0u) ^ (w & 1u) ^ (ws & 1u);
                }
            }
        }
    }
    const uint32_t toggle = flip ? 0x80000000u : 0u;
#pragma unroll
    for (int a = 0; a < 3; ++a) out[3 * i + a] = __uint_as_float(__float_as_uint(normals[3 * i + a]) ^ toggle);
    flipped[i] = (uint8_t)flip;
}

inline bool or_count(int64_t n) { return n >= 1 && n <= UP_MAX_ITEMS; }
inline bool or_k(int32_t k) { return k >= 1 && k <= BS_PC_KNN_MAX; }
inline dim3 or_grid(int64_t n) { return dim3((unsigned)cdiv64(n, OR_THREADS)); }

}  // namespace
}  // namespace bs

#define OR_ENTER(name)                                                                 \
    using namespace bs;                                                                \
    if (!initialized()) { set_error(name ": call bs_init first"); return BS_ERR_NOT_INIT; } \
    hipStream_t st = reinterpret_cast<hipStream_t>(stream)

extern "C" int bs_pc_orient_edges(const float* points, const float* normals, int64_t n, const int32_t* index, const int32_t* count, int32_t k,
                                  void* keys, int32_t* valid, void* stream) {
    OR_ENTER("bs_pc_orient_edges");
    BS_REQUIRE(points && normals && index && count && keys && valid, "bs_pc_orient_edges: null pointer");
    BS_REQUIRE(or_count(n) && or_k(k), "bs_pc_orient_edges: n = %lld (1 <= n <= 2^30), k = %d (1 <= k <= %d)", (long long)n, k, BS_PC_KNN_MAX);
    BS_REQUIRE(((uintptr_t)keys & 7) == 0, "bs_pc_orient_edges: keys must be 8-byte aligned");
    hipLaunchKernelGGL(pc_orient_edges_kernel, or_grid(n * k), dim3(OR_THREADS), 0, st, points, normals, n, index, count, (int)k,
                       static_cast<or_key*>(keys), valid);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_pc_orient_clear(void* best, int32_t* best_hi, int64_t n, void* stream) {
    OR_ENTER("bs_pc_orient_clear");
    BS_REQUIRE(best && or_count(n) && ((uintptr_t)best & 7) == 0, "bs_pc_orient_clear: best %p (8-byte aligned), n = %lld", best, (long long)n);
    hipLaunchKernelGGL(pc_orient_clear_kernel, or_grid(n), dim3(OR_THREADS), 0, st, static_cast<or_key*>(best), best_hi, n);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_pc_orient_select(const void* keys, const int32_t* index, const uint32_t* word, int64_t n, int32_t k, void* best, int32_t* crossing,
                                   void* stream) {
    OR_ENTER("bs_pc_orient_select");
    BS_REQUIRE(keys && index && word && best && crossing, "bs_pc_orient_select: null pointer");
    BS_REQUIRE(or_count(n) && or_k(k), "bs_pc_orient_select: n = %lld, k = %d", (long long)n, k);
    BS_REQUIRE((((uintptr_t)keys | (uintptr_t)best) & 7) == 0, "bs_pc_orient_select: keys and best must be 8-byte aligned");
    hipLaunchKernelGGL(pc_orient_select_kernel, or_grid(n * k), dim3(OR_THREADS), 0, st, static_cast<const or_key*>(keys), index, word, n, (int)k,
                       static_cast<or_key*>(best), crossing);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_pc_orient_select_hi(const void* keys, const int32_t* index, const uint32_t* word, int64_t n, int32_t k, const void* best,
                                      int32_t* best_hi, void* stream) {
    OR_ENTER("bs_pc_orient_select_hi");
    BS_REQUIRE(keys && index && word && best && best_hi, "bs_pc_orient_select_hi: null pointer");
    BS_REQUIRE(or_count(n) && or_k(k), "bs_pc_orient_select_hi: n = %lld, k = %d", (long long)n, k);
    BS_REQUIRE((((uintptr_t)keys | (uintptr_t)best) & 7) == 0, "bs_pc_orient_select_hi: keys and best must be 8-byte aligned");
    hipLaunchKernelGGL(pc_orient_select_hi_kernel, or_grid(n * k), dim3(OR_THREADS), 0, st, static_cast<const or_key*>(keys), index, word, n, (int)k,
                       static_cast<const or_key*>(best), best_hi);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_pc_orient_hook(const float* normals, uint32_t* word, int64_t n, const void* best, const int32_t* best_hi, void* stream) {
    OR_ENTER("bs_pc_orient_hook");
    BS_REQUIRE(normals && word && best && best_hi && or_count(n), "bs_pc_orient_hook: null pointer or n = %lld", (long long)n);
    BS_REQUIRE(((uintptr_t)best & 7) == 0, "bs_pc_orient_hook: best must be 8-byte aligned");
    hipLaunchKernelGGL(pc_orient_hook_kernel, or_grid(n), dim3(OR_THREADS), 0, st, normals, word, n, static_cast<const or_key*>(best), best_hi);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_pc_orient_compress(uint32_t* word, int64_t n, void* stream) {
    OR_ENTER("bs_pc_orient_compress");
    BS_REQUIRE(word && or_count(n), "bs_pc_orient_compress: word %p, n = %lld", (void*)word, (long long)n);
    hipLaunchKernelGGL(pc_orient_compress_kernel, or_grid(n), dim3(OR_THREADS), 0, st, word, n);
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_pc_orient_seed(const float* points, const int32_t* valid, const uint32_t* word, int64_t n, void* seed, void* stream) {
    OR_ENTER("bs_pc_orient_seed");
    BS_REQUIRE(points && valid && word && seed && or_count(n), "bs_pc_orient_seed: null pointer or n = %lld", (long long)n);
    BS_REQUIRE(((uintptr_t)seed & 7) == 0, "bs_pc_orient_seed: seed must be 8-byte aligned");
    hipLaunchKernelGGL(pc_orient_seed_kernel, or_grid(n), dim3(OR_THREADS), 0, st, points, valid, word, n, static_cast<or_key*>(seed));
    BS_CHECK_LAUNCH();
    return BS_OK;
}

extern "C" int bs_pc_orient_flip(const float* normals, const int32_t* valid, const uint32_t* word, int64_t n, const void* seed, double dx, double dy,
                                 double dz, float* out, uint8_t* flipped, void* stream) {
    OR_ENTER("bs_pc_orient_flip");
    BS_REQUIRE(normals && valid && word && seed && out && flipped && or_count(n), "bs_pc_orient_flip: null pointer or n = %lld", (long long)n);
    BS_REQUIRE(out != normals, "bs_pc_orient_flip: out must not alias normals");
    BS_REQUIRE(isfinite(dx) && isfinite(dy) && isfinite(dz), "bs_pc_orient_flip: direction (%g, %g, %g)", dx, dy, dz);
    BS_REQUIRE(((uintptr_t)seed & 7) == 0, "bs_pc_orient_flip: seed must be 8-byte aligned");
    hipLaunchKernelGGL(pc_orient_flip_kernel, or_grid(n), dim3(OR_THREADS), 0, st, normals, valid, word, n, static_cast<const or_key*>(seed), dx, dy, dz,
                       out, flipped);
    BS_CHECK_LAUNCH();
    return BS_OK;
}
