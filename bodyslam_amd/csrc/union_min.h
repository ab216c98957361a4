// Union by minimum over an int32 parent array, shared by the mesh components (mesh_ops.hip, bs_mesh_cc_*) and the DBSCAN clusters
// (radius.hip, bs_pc_dbscan_*): one copy of the root walk, the hook and the compression, so the two cannot drift apart.
//   parent [n] starts as 0 .. n - 1 and is only ever lowered (atomicMin of a smaller root into a larger root's slot), so parent[x] <= x
//   always: a root walk strictly descends -- at most n steps, no spin, no retry loop.  The caller repeats (hook every edge, compress) until
//   a hook round reports no change; every round that reports one turns at least one root into a non-root for good, so at most n rounds do.
//   At the fixed point every member of a component has the same root, and since root(x) <= x it is the component's smallest index: unique
//   whatever the schedule.  Integer atomics only.
#pragma once
#include "common.h"

namespace bs {

// the root of x: parent[p] <= p, so every step strictly descends and there are at most n of them
__device__ __forceinline__ int32_t cc_root(const int32_t* parent, int32_t x, int64_t n) {
    for (int64_t step = 0; step < n; ++step) {
        const int32_t p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p >= x || p < 0) break;
        x = p;
    }
    return x;
}

// the hook of one edge (a, b), both in [0, n): when the roots differ, the smaller one goes into the larger one's slot
__device__ __forceinline__ void cc_union(int32_t* parent, int32_t a, int32_t b, int64_t n, int32_t* __restrict__ changed) {
    const int32_t ra = cc_root(parent, a, n), rb = cc_root(parent, b, n);
    if (ra == rb) return;
    atomicMin(&parent[ra > rb ? ra : rb], ra > rb ? rb : ra);
    *changed = 1;                                                    // (every writer stores the same value)
}

// parent[x] = root(x): a root stays a root during a launch of these, and every value a walk can meet lies on the path to it
__device__ __forceinline__ void cc_compress(int32_t* parent, int32_t x, int64_t n) {
    __hip_atomic_store(&parent[x], cc_root(parent, x, n), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace bs
