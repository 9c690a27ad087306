// lds_plan.h — how a traversal kernel's dynamic LDS is split between the
// top-of-tree node cache and the per-thread BVH4 stacks.  Pure host code, no
// HIP: both launchers and bind.cpp (C.lds_plan, tests/test_lds_plan.py) use it.
#pragma once
#include <cstdint>

namespace hippt {

constexpr int LDS_BLOCK = 256;                  // threads of every render block
constexpr int LDS_ENTRY_BYTES = LDS_BLOCK * 8;  // one stack entry per thread
constexpr int LDS_MIN_STACK = 4;                // entries the cache must leave

// Stack entries of LDS per block that keep `occ` waves/SIMD resident: the
// block allocation is the occupancy governor (3:26, 4:20, 5:16, 6 and up:12).
constexpr int lds_entries(int occ) {
    return occ <= 3 ? 26 : occ == 4 ? 20 : occ == 5 ? 16 : 12;
}

// Block layout: [n_cached nodes][lds_n stack entries x 256 threads].
struct LdsPlan { int lds_n, n_cached; uint32_t shmem; };

// The cache takes its share of the budget first, capped so that LDS_MIN_STACK
// stack entries remain; the stacks get the rest (deeper pushes go to private
// memory).  lds_req in [0, lds_max) asks for fewer stack entries (ray probe).
// A stack in scratch has lds_n = 0; `scratch_drops_cache` then drops the
// cache too, otherwise the cache keeps the size it has beside an LDS stack.
inline LdsPlan lds_plan(int occ, bool stack_in_lds, bool scratch_drops_cache,
                        int n_nodes4, int node_bytes, int cache_req, int lds_req = -1) {
    LdsPlan p{0, 0, 0};
    if (!stack_in_lds && scratch_drops_cache) return p;
    const int budget = lds_entries(occ) * LDS_ENTRY_BYTES;
    const int cache_cap = (budget - LDS_MIN_STACK * LDS_ENTRY_BYTES) / node_bytes;
    p.n_cached = cache_req < n_nodes4 ? cache_req : n_nodes4;
    if (p.n_cached > cache_cap) p.n_cached = cache_cap;
    if (p.n_cached < 0) p.n_cached = 0;
    if (stack_in_lds) {
        const int lds_max = (budget - p.n_cached * node_bytes) / LDS_ENTRY_BYTES;
        p.lds_n = lds_req >= 0 && lds_req < lds_max ? lds_req : lds_max;
    }
    p.shmem = (uint32_t)(p.lds_n * LDS_ENTRY_BYTES + p.n_cached * node_bytes);
    return p;
}

} // namespace hippt
