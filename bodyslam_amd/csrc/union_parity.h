// Union by minimum with one parity bit per link, beside union_min.h: the components of a graph whose links (a, b, s) each state
// flip(a) xor flip(b) = s -- the orientation of normals along a spanning tree (orient.hip, bs_pc_orient_*) and the winding of a mesh
// (mesh_ops.hip, bs_mesh_orient_*).  union_min.h's schedule-free half carries over word for word; this adds the parity half once.
//   word [n], one 32-bit word per item: parent << 1 | parity, parity = flip(x) xor flip(parent).  It starts as x << 1 (every item its own
//   root, parity 0) and is only ever lowered: atomicMin of (smaller root << 1 | parity) into the larger root's slot.  The parent is the high
//   part, so a lower word never has a higher parent: parent <= x always, a root walk strictly descends -- at most n steps, no spin, no
//   retry loop.  Items number at most 2^30 (UP_MAX_ITEMS), so that parent << 1 fits and the order of the words is the order of the parents.
//   THE INVARIANT: every stored word is a relation implied by the links hooked so far.  It holds at the start (flip(x) xor flip(x) = 0).  A
//   walk from a xors the parities it meets, so what it returns -- wherever it stops, whatever other threads store meanwhile -- is an implied
//   relation between a and the item it stopped at; the hook of (a, b, s) stores flip(ra) xor flip(rb) = pa xor pb xor s, which those two
//   and the link imply; atomicMin keeps one of two implied words; compression stores (root << 1 | parity to the root), the xor of a walk.
//   IT FOLLOWS that on a consistent link set -- one with a flip assignment that satisfies every link, which a tree always is -- every
//   implied relation between two items of a component has one value, so at the fixed point every item's parity to its component's smallest
//   index is the same under every schedule.  On an inconsistent set the words are still implied relations, but which ones depends on the
//   schedule: the caller re-tests every link against the stored parities (bs_mesh_orient_check) and uses the parities only where all hold.
//   A hook that finds its slot already lowered by a smaller root is not an error: its link is dropped for this round and hooked again by
//   the caller's next one, as in union_min.h.  Integer atomics only.
#pragma once
#include "common.h"

namespace bs {

constexpr int64_t UP_MAX_ITEMS = (int64_t)1 << 30;

// the root of x < n and, in `parity`, flip(x) xor flip(root): the parent of every word met is below the item, so every index stays in [0, n)
__device__ __forceinline__ uint32_t up_root(const uint32_t* word, uint32_t x, int64_t n, uint32_t& parity) {
    uint32_t par = 0;
    for (int64_t step = 0; step < n; ++step) {
        const uint32_t w = __hip_atomic_load(&word[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((w >> 1) >= x) break;
        par ^= w & 1u;
        x = w >> 1;
    }
    parity = par;
    return x;
}

// the hook of one link (a, b, s), a and b in [0, n): when the roots differ, (the smaller root << 1 | pa ^ pb ^ s) goes into the larger one's
// slot by atomicMin.  -> whether the roots differed
__device__ __forceinline__ bool up_union(uint32_t* word, uint32_t a, uint32_t b, uint32_t s, int64_t n) {
    uint32_t pa, pb;
    const uint32_t ra = up_root(word, a, n, pa), rb = up_root(word, b, n, pb);
    if (ra == rb) return false;
    atomicMin(&word[ra > rb ? ra : rb], ((ra > rb ? rb : ra) << 1) | ((pa ^ pb ^ s) & 1u));
    return true;
}

// word[x] = root(x) << 1 | parity to the root: a root stays a root during a launch of these, and every word a walk can meet is implied
__device__ __forceinline__ void up_compress(uint32_t* word, uint32_t x, int64_t n) {
    uint32_t par;
    const uint32_t r = up_root(word, x, n, par);
    __hip_atomic_store(&word[x], (r << 1) | par, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace bs
