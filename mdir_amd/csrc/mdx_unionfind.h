// The lock-free union-find of the near-duplicate groups (include/mdx.h, "near-duplicate groups"), written once for the device
// (mdx_groups.hip) and for the host program that tests the algorithm itself from several threads (tests/unionfind_host.cpp).
//
// Forest.  parent[x] <= x at all times; a root has parent[x] == x.  Only a root is ever hooked, by a compare-and-swap that
// expects the root's own id, and always under a SMALLER id: the root of every tree is the minimum of the tree, and once every
// edge is in, each component is one tree whose root is the label.  Path halving lowers parent[x] to an ancestor and nothing
// else (store_min of an ancestor: the smaller of two ancestors of x is an ancestor of x), so a value read at any time, however
// stale, is still an ancestor of x -- the walk from it ends in the same tree.  A hook by an atomic min on a non-root would be
// shorter and wrong: it can replace a link that another thread's walk has just passed and drop the subtree above it.
//
// Memory policy M (all three on one int32 word; what the device's are is said in mdx_groups.hip):
//   M::load(p)                     the value of *p, never one cached from before another thread's store
//   M::cas(p, expected, desired)   the value *p held; the swap happened iff that equals `expected`
//   M::store_min(p, v)             *p = min(*p, v), atomically
//
// A failed cas is never followed by a fresh load of the same word: the retry continues from the value the cas returned.  A
// load that could return the same stale "I am a root" for ever, against a cas that sees the true value, would never end.
//
// Bounded loops.  A walk visits strictly decreasing ids, so it ends within n steps; a retry of unite follows a hook of the same
// root by another thread, and a level has at most n - 1 hooks.  Both loops still count, and past `limit` (n + 1) they give up:
// MDX_UF_GAVE_UP is returned and nothing is hooked.  A parent outside [0, x] (a forest that mdx_groups_init did not write) gives
// up at once, before it is used as an index.  Nothing here waits for another thread.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MDX_UF_FN __host__ __device__ __forceinline__
#else
#define MDX_UF_FN inline
#endif

namespace mdx {

constexpr int MDX_UF_GAVE_UP = 1;       // bit 0 of the status flags

// the root of x's tree (a moment ago), halving the path on the way; flags |= MDX_UF_GAVE_UP where the walk was abandoned (the
// id it had reached is returned: an ancestor, not necessarily a root)
template <class M> MDX_UF_FN int32_t uf_find(int32_t *parent, int32_t x, int64_t limit, int &flags)
{
    int32_t p = M::load(parent + x);
    for (int64_t step = 0; p != x; ++step) {
        if ((uint32_t)p > (uint32_t)x || step > limit) {
            flags |= MDX_UF_GAVE_UP;
            return x;
        }
        const int32_t gp = M::load(parent + p);
        if ((uint32_t)gp < (uint32_t)p) M::store_min(parent + x, gp);       // halving: x now points to its grandparent, or lower
        x = p;
        p = gp;
    }
    return x;
}

// the same walk without a store, for a forest nobody writes any more (the label pass): the root, or the id reached at `limit`
template <class M> MDX_UF_FN int32_t uf_root(const int32_t *parent, int32_t x, int64_t limit)
{
    for (int64_t step = 0; step <= limit; ++step) {
        const int32_t p = M::load(const_cast<int32_t *>(parent) + x);
        if ((uint32_t)p >= (uint32_t)x) break;
        x = p;
    }
    return x;
}

// joins the trees of a and b; returns 1 when this call made the hook, 0 when they were (or have meanwhile become) one tree or
// the call gave up
template <class M> MDX_UF_FN int uf_unite(int32_t *parent, int32_t a, int32_t b, int64_t limit, int &flags)
{
    for (int64_t tries = 0; tries <= limit; ++tries) {
        a = uf_find<M>(parent, a, limit, flags);
        b = uf_find<M>(parent, b, limit, flags);
        if (a == b || (flags & MDX_UF_GAVE_UP)) return 0;
        const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const int32_t seen = M::cas(parent + hi, hi, lo);
        if (seen == hi) return 1;
        if ((uint32_t)seen > (uint32_t)hi) break;                            // not a forest of mdx_groups_init
        a = seen;                      // hi was hooked by someone else, under `seen`: go on from there, not from a fresh load
        b = lo;
    }
    flags |= MDX_UF_GAVE_UP;
    return 0;
}

}  // namespace mdx
