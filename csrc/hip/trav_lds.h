// trav_lds.h — what the megakernel and the wavefront launchers share: the
// environment knobs, the top-cache request and the kernels' LDS prologue.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>
#include "lds_plan.h"
#include "../core/scene_view.h"

namespace hippt {

// A/B hooks.  Callers keep the value in a function-local static, so every
// variable is read once per process.
inline int env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}
inline bool env_is(const char* name, const char* value) {
    const char* e = getenv(name);
    return e && strcmp(e, value) == 0;
}

// Leading nodes of the traversal array to copy into LDS per block.  Priority:
// probe argument > HIPPT_TOPCACHE (A/B hook) > accelerator XML cache_level >
// measured default 64 (8 KB; 128 measured +1.0 Msamples/s on the kitchen,
// inside the noise bar, for four more stack entries' worth of LDS).
// lds_plan() clamps the request.
inline int top_cache_request(const SceneView& sv, int probe = -1) {
    static const int cache_env = env_int("HIPPT_TOPCACHE", -1);
    return probe >= 0 ? probe : cache_env >= 0 ? cache_env
         : sv.cache_nodes > 0 ? sv.cache_nodes : 64;
}

// Bytes one cached node occupies (TRAV_CACHE_STRIDE, bvh4.h): what both
// launchers hand to lds_plan as node_bytes, so that the plan budgets what
// the cache really takes, padding included in a HIPPT_CACHE_STRIDE=144 build.
constexpr int TRAV_CACHE_NODE_BYTES = bvh_cache_stride<TravNode>();

// Dynamic-LDS layout of every traversal kernel (lds_plan.h):
// [n_cached nodes at TRAV_CACHE_NODE_BYTES each][per-thread stacks].  The
// first n_cached nodes of the traversal array are copied into LDS once per
// block.  The host orders that array top first (bvh4_top_first, bvh4.h), so
// these are the root and the nodes most walks visit after it, not the
// depth-first head of the tree; LDS is ~4x closer than L2.  tid = the
// thread's index in its 256-block.
__device__ __forceinline__ TravCtx trav_lds_ctx(const SceneView& sv, uint64_t* s_stk,
                                                int tid, int lds_n, int n_cached) {
    constexpr int NW = (int)(sizeof(TravNode) / 8);   // u64 words per node
    constexpr int SW = TRAV_CACHE_NODE_BYTES / 8;     // u64 words per cached node
    static_assert((NW & (NW - 1)) == 0 && TRAV_CACHE_NODE_BYTES % 8 == 0, "word split");
    TravNode* s_cache = (TravNode*)s_stk;
    uint64_t* s_base = s_stk + (size_t)n_cached * SW;
    for (int i = tid; i < n_cached * NW; i += LDS_BLOCK)
        s_stk[(i / NW) * SW + (i % NW)] = ((const uint64_t*)trav_nodes(sv))[i];
    if (n_cached > 0) __syncthreads();
    return TravCtx{(LdsSlot)&s_base[tid], lds_n, s_cache, n_cached};
}

} // namespace hippt
