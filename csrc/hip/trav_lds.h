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

// Nodes of the tree top to copy into LDS per block.  Priority: probe
// argument > HIPPT_TOPCACHE (A/B hook) > accelerator XML cache_level >
// measured default 64 (8 KB).  lds_plan() clamps the request.
inline int top_cache_request(const SceneView& sv, int probe = -1) {
    static const int cache_env = env_int("HIPPT_TOPCACHE", -1);
    return probe >= 0 ? probe : cache_env >= 0 ? cache_env
         : sv.cache_nodes > 0 ? sv.cache_nodes : 64;
}

// Dynamic-LDS layout of every traversal kernel (lds_plan.h):
// [n_cached 128-byte top-tree nodes][per-thread stacks].  The top of the
// tree is copied into LDS once per block: every walk's first visits are
// nodes 0..n_cached and the walk is bound by hit LATENCY (95% L2 hit rate)
// — LDS is ~4x closer than L2.  tid = the thread's index in its 256-block.
__device__ __forceinline__ TravCtx trav_lds_ctx(const SceneView& sv, uint64_t* s_stk,
                                                int tid, int lds_n, int n_cached) {
    constexpr int NW = (int)(sizeof(TravNode) / 8);   // u64 words per node
    TravNode* s_cache = (TravNode*)s_stk;
    uint64_t* s_base = s_stk + (size_t)n_cached * NW;
    for (int i = tid; i < n_cached * NW; i += LDS_BLOCK)
        ((uint64_t*)s_cache)[i] = ((const uint64_t*)trav_nodes(sv))[i];
    if (n_cached > 0) __syncthreads();
    return TravCtx{(LdsSlot)&s_base[tid], lds_n, s_cache, n_cached};
}

} // namespace hippt
