// bvh8.h — 8-wide BVH node; its walks are the width-8 instances of bvh4.h's.
//
// Same design as bvh4.h taken one step further: a 256-byte node (4 cache
// lines) holds 8 child AABBs in SoA layout, so one step of the dependent
// walk issues 16 independent 16-byte loads and tests 8 boxes.  At the
// measured BVH4 operating point (VALUBusy 42%, VALUUtilization 20%) the
// extra slab VALU work is free; what the wider node buys is another
// halving of dependent steps per ray and more uniform per-lane iteration
// counts (wave64 divergence).  Host-tested record only: no kernel walks
// this tree (measured 2.4x slower than BVH4, scene_view.h).
#pragma once
#include "bvh4.h"

namespace hippt {

using BVH8Node = BVHWideNode<8>;
static_assert(sizeof(BVH8Node) == 256, "BVH8Node must be 256 bytes");

// bvh4_sel4 with one more level, and the child word picked through it (so
// this walk, too, keeps its node copy in registers).
HD uint32_t bvh8_sel8(const int32_t (&w)[8], uint32_t slot) {
    uint32_t a = bvh4_sel4((uint32_t)w[0], (uint32_t)w[1], (uint32_t)w[2], (uint32_t)w[3], slot);
    uint32_t b = bvh4_sel4((uint32_t)w[4], (uint32_t)w[5], (uint32_t)w[6], (uint32_t)w[7], slot);
    return (slot & 4u) ? b : a;
}
HD uint32_t bvh_child_word_at(const BVH8Node& nd, uint32_t slot) {
    return bvh4_child_word((int)bvh8_sel8(nd.child, slot), (int)bvh8_sel8(nd.cnt, slot));
}

// Closest-hit while-while walk (keys are insertion-sorted at this width).
HD HitRecord ray_intersect_bvh8_ww(const BVH8Node* nodes,
                                   const Prim* prims, const uint32_t* prim_obj,
                                   const Ray& ray, float tmax,
                                   LdsSlot lds_slot = nullptr, int lds_n = 0) {
    return bvh_closest_ww(nodes, prims, prim_obj, ray, tmax, lds_slot, lds_n,
                          (const BVH8Node*)nullptr, 0, false);
}

// Any-hit occlusion, inline leaves (unordered).
HD bool occlusion_test_bvh8(const BVH8Node* nodes,
                            const Prim* prims, const uint32_t* prim_obj,
                            const Ray& ray, float tmax,
                            LdsSlot lds_slot = nullptr, int lds_n = 0) {
    return bvh_any_inline(nodes, prims, prim_obj, ray, tmax, lds_slot, lds_n);
}

} // namespace hippt
