// The open-addressing table of 64-bit keys shared by voxel down-sampling (voxel.hip: a voxel's key) and the mesh's edge list (mesh_ops.hip:
// an edge's key): one copy of the hash, the bounded probe loop and the leader flags, so the two cannot drift apart.  The caller fills `keys`
// with SLOT_EMPTY and picks `slots`, a power of two.  What a kernel keeps per slot -- the voxel's `first`, the edge's three counters -- stays
// with that kernel: only the lookup is shared.  (tsdf.hip's block table has its own hash, signed keys and a plain load; it is not this one.)
#pragma once
#include "common.h"

namespace bs {

typedef unsigned long long slot_key;
static_assert(BS_PC_VOXEL_EMPTY_KEY == BS_MESH_EDGE_EMPTY_KEY, "the voxel table and the edge table are one table: one empty key");
constexpr slot_key SLOT_EMPTY = BS_PC_VOXEL_EMPTY_KEY;
constexpr int SLOT_THREADS = 256;

__device__ __forceinline__ slot_key slot_mix(slot_key x) {             // (which slot a key starts at changes the time only)
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

// The slot of `key`, inserted when it is new; -1 after `slots` probes: a full table costs the caller an error, never a spinning wave.  Linear
// probing from the mixed hash.  A slot goes from SLOT_EMPTY to its key once and never changes again, so a relaxed load that shows a key other
// than SLOT_EMPTY is final: only an empty slot needs the compare-and-swap.
__device__ __forceinline__ int32_t slot_insert(slot_key* __restrict__ keys, int64_t slots, slot_key key) {
    const slot_key mask = (slot_key)slots - 1;
    slot_key slot = slot_mix(key) & mask;
    int32_t found = -1;
    for (int64_t probe = 0; probe < slots; ++probe) {
        slot_key cur = __hip_atomic_load(&keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == SLOT_EMPTY) cur = atomicCAS(&keys[slot], SLOT_EMPTY, key);
        if (cur == SLOT_EMPTY || cur == key) { found = (int32_t)slot; break; }
        slot = (slot + 1) & mask;
    }
    return found;
}

// leader[i] = first[slot_of[i]] (-1 for an item without a slot), is_first[i] = (leader[i] == i).  The caller's inclusive scan of is_first
// (integer, exact) is the rank: the group led by item j has row rank[j] - 1 -- first appearance order, whatever slot the group got.
static __global__ void __launch_bounds__(SLOT_THREADS) slot_flags_kernel(const int32_t* __restrict__ slot_of, const int32_t* __restrict__ first,
                                                                         int64_t slots, int64_t n, int32_t* __restrict__ leader,
                                                                         int32_t* __restrict__ is_first) {
    const int64_t i = (int64_t)blockIdx.x * SLOT_THREADS + threadIdx.x;
    if (i >= n) return;
    const int32_t slot = slot_of[i];
    const int32_t ld = slot >= 0 && slot < slots ? first[slot] : -1;
    leader[i] = ld;
    is_first[i] = ld == (int32_t)i ? 1 : 0;
}

// (the caller has checked its arguments under its own name, and checks the launch)
static inline void slot_flags_launch(const int32_t* slot_of, const int32_t* first, int64_t slots, int64_t n, int32_t* leader, int32_t* is_first,
                                     hipStream_t st) {
    hipLaunchKernelGGL(slot_flags_kernel, dim3((unsigned)cdiv64(n, SLOT_THREADS)), dim3(SLOT_THREADS), 0, st, slot_of, first, slots, n, leader,
                       is_first);
}

}  // namespace bs
