// bvh4.h — wide BVH node layouts, the traversal pieces, and the walks built
// from them.
//
// Capability parity: same traversal semantics as the binary skip-link walk in
// bvh.h (reference src/renderer/tracing_func.cuh:44-181), but the node is
// re-designed for CDNA4 instead of copied: the binary walk is a serial
// dependent-load chain (measured VALUBusy ~4% on MI355X — the megakernel is
// latency-bound on L2/HBM, profiles/README.md), so the fix is to shorten the
// chain, not to widen the fetch of a single step (speculative dual-fetch was
// measured -18%).  A 4-wide node:
//   * is one 128-byte record = 7 independent 16-byte loads per step (the
//     traversal node BVH4NodeT: boxes + pre-tagged child words) — the
//     memory parallelism lives INSIDE one step of the dependent chain,
//   * halves tree depth (half as many dependent steps per ray),
//   * tests 4 AABBs per step with pure VALU work, which is nearly free at 4%
//     VALU utilization,
//   * enables ordered (front-to-back) traversal with a short stack — the
//     DFS skip-link layout cannot reorder children, a 4-wide stack walk can,
//     and each stack entry carries t_near so stale far subtrees are culled
//     on pop after the hit distance tightens.
//
// Layout of this file: node types, then the pieces every walk is built from
// (tagged child word, slab test, key build + sort, stack, leaf loops), each
// written once, then the walks.
//
// Form of the pieces.  Pieces over scalars and the node copy are HD
// functions.  Pieces that write the walk's private arrays or leave the walk
// from inside a loop — key build + sort, stack push and pop, the ordered
// node visit made of them, the any-hit leaf loop — are function-like macros
// (BVH_*), because a function boundary there is not code-neutral: the
// compiler simplifies a helper on its own before it inlines it, where `keys`
// and `stack` are opaque pointers and not yet the caller's promotable
// locals, and the walk comes out differently (as HD functions ScratchSize
// moved in 14 of 45 kernels, e.g. k_render<0,4,false> 1216 -> 1232 B/lane;
// scripts/kernel_resources.py).  As macros, every kernel except the
// bvh-cost visualiser is instruction for instruction what the hand-copied
// walks compiled to (profiles/README.md).
//
// Since the node copy stays in registers the walk is bound by instruction
// issue, not by latency (VALUBusy 71% at ~13 of 64 lanes active), so the
// device walks run on BVH4NodeT and visit it with BVH_VISIT_TAGGED4, the
// branch-free width-4 form of the ordered visit; the BVH4Node forms stay for
// the host walks, width 8 and as the other side of C.bvh4_visit_selftest.
// What latency is left sits in the leaf loops, which therefore read the
// whole primitive at once and wait for it once (bvh_load_prim).
//
// Which walks a kernel can reach in the default build:
//   ray_intersect_bvh4_ww, occlusion_test_bvh4_ww   every render kernel
//   bvh4_walk_step                                  k_wf_trace_dual
//   bvh4_cost                                       bvh-cost renderer only
// Everything else is a host-tested record or A/B oracle: the inline-leaf
// walks ray_intersect_bvh4 / occlusion_test_bvh4, the quantized *q_ww walks
// (device code only when built with HIPPT_QBVH=1), and the 8-wide walks of
// bvh8.h.
#pragma once
#include <queue>
#include <stdexcept>
#include <vector>
#include "bvh.h"

namespace hippt {

// W-wide node, 32*W bytes.  Box storage is SoA-within-node (lo_x[W],
// lo_y[W], ...) so the W slab tests read same-stride floats from the same
// cache lines.
//   child[c] >= 0 : internal child, index of a node
//   child[c] <  0 : leaf child, prim_base = ~child[c], prim count = cnt[c]
//   child[c] <  0 AND cnt[c] == 0: empty slot (collapse_bvh4 writes ~0 and a
//                   far-away point box, so it is almost never hit either)
// The walks apply the empty-slot rule (a leaf child of no prims is dropped)
// after the slab test, so it is paid only for children whose box is hit.
template <int W>
struct alignas(16) BVHWideNode {
    static constexpr int WIDTH = W;
    static constexpr bool EMPTY_BEFORE_BOX = false;
    static constexpr bool TAGGED = false;
    float lo_x[W], lo_y[W], lo_z[W];
    float hi_x[W], hi_y[W], hi_z[W];
    int32_t child[W];
    int32_t cnt[W];
};
using BVH4Node = BVHWideNode<4>;
static_assert(sizeof(BVH4Node) == 128, "BVH4Node must be 128 bytes");

// Traversal node: the BVH4Node the device walks load.  Same boxes; in place
// of child[] it stores the tagged word of every slot (bvh4_child_word below:
// BVH4_NONE_W for an empty slot or a leaf of no prims), so a visit neither
// loads cnt[] nor builds words — 7 x 16-byte loads instead of 8.  The last
// 16 bytes are padding no walk loads: the record stays 128 bytes so that no
// node straddles a cache line.  Made once per scene from the BVH4Node array
// (tag_bvh4 at the end of this file); builders, the scene cache and the
// inline host walks stay on BVH4Node.
struct alignas(16) BVH4NodeT {
    static constexpr int WIDTH = 4;
    static constexpr bool EMPTY_BEFORE_BOX = false;
    static constexpr bool TAGGED = true;
    float lo_x[4], lo_y[4], lo_z[4];
    float hi_x[4], hi_y[4], hi_z[4];
    uint32_t child[4];       // tagged child words
    uint32_t pad[4];
};
static_assert(sizeof(BVH4NodeT) == 128, "BVH4NodeT must be 128 bytes");

// Quantized 64-byte 4-wide node (Ylitie-style child-box compression,
// re-derived for this tree): child AABBs stored as uint8 offsets inside
// the node's own box, power-of-two per-axis scales so decompression is
// an fma per bound.  Quantized bounds round OUTWARD (conservative: never
// misses a hit, a few extra visits).  Halves bytes per dependent node
// load (1 cacheline, not 2) and doubles LDS top-cache coverage.
// An empty slot is known by its word, before the box is dequantized.
struct alignas(16) BVH4NodeQ {
    static constexpr int WIDTH = 4;
    static constexpr bool EMPTY_BEFORE_BOX = true;
    static constexpr bool TAGGED = true;
    float ox, oy, oz;       // node box origin
    uint8_t ex, ey, ez;      // per-axis scale exponents: scale = 2^(e-127)
    uint8_t pad;
    uint8_t qlo[4][3];       // child lo offsets (floor)
    uint8_t qhi[4][3];       // child hi offsets (ceil); qhi<qlo = empty slot
    uint32_t child[4];       // tagged child words (BVH4_NONE_W for empty)
};
static_assert(sizeof(BVH4NodeQ) == 64, "BVH4NodeQ must be 64 bytes");

constexpr int BVH4_STACK = 64;  // >= 3 * max collapsed depth; checked at build

// ------------------------------------------------------------ tagged word
// The form traversal stacks and `cur` carry: bit31 = leaf, [30:27] = prim
// count (builders cap leaves at 15 prims), [26:0] = prim base (up to 134M
// prims); or the plain node index.  BVH4_NONE_W is neither: it stands for an
// empty child slot and for "nothing left to visit".
constexpr uint32_t BVH4_NONE_W = 0x7fffffffu;
HD uint32_t bvh4_filled_word(int ch, int pc) {  // of a slot known not to be empty
    return ch < 0 ? (0x80000000u | ((uint32_t)pc << 27) | (uint32_t)(~ch)) : (uint32_t)ch;
}
HD uint32_t bvh4_child_word(int ch, int pc) {
    if (ch < 0 && pc == 0) return BVH4_NONE_W;  // the empty-slot rule
    return bvh4_filled_word(ch, pc);
}
HD bool bvh4_is_leaf(uint32_t w) { return w >= 0x80000000u; }
HD bool bvh4_not_leaf(uint32_t w) { return w < 0x80000000u; }  // node or NONE
HD bool bvh4_is_node(uint32_t w) { return bvh4_not_leaf(w) && w != BVH4_NONE_W; }
HD int bvh4_leaf_base(uint32_t w) { return (int)(w & 0x07ffffffu); }
HD int bvh4_leaf_count(uint32_t w) { return (int)((w >> 27) & 0xfu); }

// w[slot] as a select tree over registers.  The ordered walks pick the
// sorted child's fields with this instead of indexing the node copy with the
// run-time slot: nd.child[keys[k] & 3] forces the whole node copy into a
// private-memory slot — stored on every visit, re-loaded once per hit child —
// on the dependent chain between the last slab test and the next node index.
HD uint32_t bvh4_sel4(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3,
                      uint32_t slot) {
    uint32_t a = (slot & 1u) ? w1 : w0;
    uint32_t b = (slot & 1u) ? w3 : w2;
    return (slot & 2u) ? b : a;
}
// Tagged word of the child in `slot` of `nd` (all node indices constant).
// Selecting child/cnt first and tagging the one word measured faster than
// tagging all four next to the slab tests and selecting the word
// (profiles/README.md): the compiler sinks the four taggings behind the
// sort, where they lengthen the chain more than the second select does.
// That holds for the BVH4Node visits, which build the word from child and
// cnt; a tagged node stores its words, and BVH_VISIT_TAGGED4 takes all four
// through the sort with no select at all.
// (bvh8.h adds the width-8 overload.)
HD uint32_t bvh_child_word_at(const BVH4Node& nd, uint32_t slot) {
    int ch = (int)bvh4_sel4((uint32_t)nd.child[0], (uint32_t)nd.child[1],
                            (uint32_t)nd.child[2], (uint32_t)nd.child[3], slot);
    int pc = (int)bvh4_sel4((uint32_t)nd.cnt[0], (uint32_t)nd.cnt[1],
                            (uint32_t)nd.cnt[2], (uint32_t)nd.cnt[3], slot);
    return bvh4_child_word(ch, pc);
}
HD uint32_t bvh_child_word_at(const BVH4NodeQ& nd, uint32_t slot) {
    return bvh4_sel4(nd.child[0], nd.child[1], nd.child[2], nd.child[3], slot);
}
HD uint32_t bvh_child_word_at(const BVH4NodeT& nd, uint32_t slot) {
    return bvh4_sel4(nd.child[0], nd.child[1], nd.child[2], nd.child[3], slot);
}
// Word of child c (a constant) of a slot already known not to be empty.
template <int W>
HD uint32_t bvh_filled_child_word(const BVHWideNode<W>& nd, int c) {
    return bvh4_filled_word(nd.child[c], nd.cnt[c]);
}
HD uint32_t bvh_filled_child_word(const BVH4NodeQ& nd, int c) { return nd.child[c]; }
HD uint32_t bvh_filled_child_word(const BVH4NodeT& nd, int c) { return nd.child[c]; }

// -------------------------------------------------------------- slab test
// Box [lo, hi] against the ray (inv_d, o_div = o * inv_d) on [0, tmax]: the
// ray is inside for t in [enter, exit_], which is empty on a miss.  The
// comparison stays with the caller: the ordered walks take `enter <= exit_`
// as a hit, the unordered ones skip on `enter > exit_`.
HD void bvh_slab(float lx, float ly, float lz, float hx, float hy, float hz,
                 const Vec3& inv_d, const Vec3& o_div, float tmax,
                 float& enter, float& exit_) {
    float t0x = fmaf(lx, inv_d.x, -o_div.x);
    float t1x = fmaf(hx, inv_d.x, -o_div.x);
    float t0y = fmaf(ly, inv_d.y, -o_div.y);
    float t1y = fmaf(hy, inv_d.y, -o_div.y);
    float t0z = fmaf(lz, inv_d.z, -o_div.z);
    float t1z = fmaf(hz, inv_d.z, -o_div.z);
    enter = fmaxf(fmaxf(fminf(t0x, t1x), fminf(t0y, t1y)),
                  fmaxf(fminf(t0z, t1z), 0.f));
    exit_ = fminf(fminf(fmaxf(t0x, t1x), fmaxf(t0y, t1y)),
                  fminf(fmaxf(t0z, t1z), tmax));
}
// Child c of a node.  bvh_slot_known_empty: can the slot be skipped before
// its box is looked at?  Never for an fp32 node (EMPTY_BEFORE_BOX is false).
template <int W>
HD bool bvh_slot_known_empty(const BVHWideNode<W>&, int) { return false; }
template <int W>
HD void bvh_child_slab(const BVHWideNode<W>& nd, int c, const Vec3& inv_d,
                       const Vec3& o_div, float tmax, float& enter, float& exit_) {
    bvh_slab(nd.lo_x[c], nd.lo_y[c], nd.lo_z[c], nd.hi_x[c], nd.hi_y[c], nd.hi_z[c],
             inv_d, o_div, tmax, enter, exit_);
}
HD bool bvh_slot_known_empty(const BVH4NodeT&, int) { return false; }
HD void bvh_child_slab(const BVH4NodeT& nd, int c, const Vec3& inv_d,
                       const Vec3& o_div, float tmax, float& enter, float& exit_) {
    bvh_slab(nd.lo_x[c], nd.lo_y[c], nd.lo_z[c], nd.hi_x[c], nd.hi_y[c], nd.hi_z[c],
             inv_d, o_div, tmax, enter, exit_);
}
// scale = 2^(e-127): e chosen so extent/255 <= scale (exact for
// power-of-two extents, <2x conservative otherwise)
HD float bvh4q_scale(uint8_t e) {
    return uint_as_float((uint32_t)(e) << 23);
}
// Quantized child: dequantized (cvt + fma per bound), then the same test.
HD bool bvh_slot_known_empty(const BVH4NodeQ& nd, int c) { return nd.child[c] == BVH4_NONE_W; }
HD void bvh_child_slab(const BVH4NodeQ& nd, int c, const Vec3& inv_d,
                       const Vec3& o_div, float tmax, float& enter, float& exit_) {
    const float sx = bvh4q_scale(nd.ex), sy = bvh4q_scale(nd.ey), sz = bvh4q_scale(nd.ez);
    bvh_slab(fmaf((float)nd.qlo[c][0], sx, nd.ox), fmaf((float)nd.qlo[c][1], sy, nd.oy),
             fmaf((float)nd.qlo[c][2], sz, nd.oz), fmaf((float)nd.qhi[c][0], sx, nd.ox),
             fmaf((float)nd.qhi[c][1], sy, nd.oy), fmaf((float)nd.qhi[c][2], sz, nd.oz),
             inv_d, o_div, tmax, enter, exit_);
}

// ---------------------------------------------------- key build and sort
// BVH_HIT_KEYS(Node, nd, inv_d, o_div, tmax, keys, nhit): slab-test the
// children of nd (a Node); declares keys[0..nhit) = the hit ones, nearest
// first.  key = (t_near bits & ~(W-1)) | slot: t_near >= 0, so the float bit
// pattern orders like the float, and the low bits carry the slot index.
// Width 4 sorts with a network, width 8 by insertion.
#define BVH_KEY_ORDER(a, b) \
    if ((a) > (b)) { uint32_t t_ = (a); (a) = (b); (b) = t_; }
#define BVH_HIT_KEYS(Node, nd, inv_d, o_div, tmax, keys, nhit)                     \
    uint32_t keys[Node::WIDTH];                                                    \
    int nhit = 0;                                                                  \
    _Pragma("unroll")                                                              \
    for (int c_ = 0; c_ < Node::WIDTH; ++c_) {                                     \
        if (bvh_slot_known_empty(nd, c_)) continue;                                \
        float enter_, exit_;                                                       \
        bvh_child_slab(nd, c_, inv_d, o_div, tmax, enter_, exit_);                 \
        if (enter_ <= exit_)                                                       \
            keys[nhit++] = (float_as_uint(enter_) & ~(Node::WIDTH - 1u)) | (uint32_t)c_; \
    }                                                                              \
    if constexpr (Node::WIDTH == 4) {                                              \
        if (nhit > 1) {                                                            \
            BVH_KEY_ORDER(keys[0], keys[1])                                        \
            if (nhit > 2) {                                                        \
                BVH_KEY_ORDER(keys[1], keys[2])                                    \
                BVH_KEY_ORDER(keys[0], keys[1])                                    \
                if (nhit > 3) {                                                    \
                    BVH_KEY_ORDER(keys[2], keys[3])                                \
                    BVH_KEY_ORDER(keys[1], keys[2])                                \
                    BVH_KEY_ORDER(keys[0], keys[1])                                \
                }                                                                  \
            }                                                                      \
        }                                                                          \
    } else {                                                                       \
        for (int i_ = 1; i_ < nhit; ++i_) {                                        \
            uint32_t k_ = keys[i_];                                                \
            int j_ = i_ - 1;                                                       \
            while (j_ >= 0 && keys[j_] > k_) { keys[j_ + 1] = keys[j_]; --j_; }    \
            keys[j_ + 1] = k_;                                                     \
        }                                                                          \
    }

// ------------------------------------------------------------------ stack
// Bottom lds_n entries live in LDS (device kernels pass a per-thread slot
// pointer into a __shared__ array, entry d at slot[d*256] for 256-thread
// blocks), the rest spill to a private (scratch) overflow array.
// Scratch-backed stacks were measured to be the BVH4 bottleneck on MI355X
// (the walk is latency-bound; per-step 8-byte scratch push/pops thrash the
// vector caches), and the LDS allocation doubles as the occupancy governor:
// LDSN entries/thread x 8 B x 256 threads of LDS per block caps blocks/CU
// exactly where the scratch walk wants to run.  On the host (lds_n = 0)
// everything goes to the plain array.
//
// Ordered walks store (t_near bits << 32) | tagged word, so that on pop
// entries whose t_near is already beyond the current hit are skipped without
// a node load; unordered walks store the bare word.
constexpr int BVH4_LDS_STRIDE = 256;  // all render blocks are 256 threads
// The per-thread slot pointer.  Under device compilation it is an
// address-space-3 pointer: through a generic pointer a pop is a flat load
// behind a run-time choice between the shared and the private aperture and a
// wait on both counters; typed, the LDS half of push and pop is a plain
// ds_write_b64 / ds_read_b64.  Kernels cast their __shared__ address once,
// where they fill in TravCtx.  On the host it is a plain pointer.
#if HIPPT_ON_DEVICE
using LdsSlot = __attribute__((address_space(3))) uint64_t*;
#else
using LdsSlot = uint64_t*;
#endif
// A host buffer standing in for a thread's LDS slots (the self-tests of
// bind.cpp; the cast exists for the device pass over that host code).
HD LdsSlot bvh_host_slot(uint64_t* p) { return (LdsSlot)p; }

#define BVH_PUSH(stack, sp, lds_slot, lds_n, e)                       \
    {                                                                 \
        if ((sp) < (lds_n)) (lds_slot)[(sp) * BVH4_LDS_STRIDE] = (e); \
        else (stack)[(sp) - (lds_n)] = (e);                           \
        ++(sp);                                                       \
    }
// Expression: the top entry.  The stack must not be empty.
#define BVH_POP(stack, sp, lds_slot, lds_n) \
    (--(sp), (sp) < (lds_n) ? (lds_slot)[(sp) * BVH4_LDS_STRIDE] : (stack)[(sp) - (lds_n)])
// cur = word of the top entry, BVH4_NONE_W if there is none.  `then_none`
// (and `then_word` below) say how the caller goes on: break, or return.
#define BVH_POP_WORD(cur, stack, sp, lds_slot, lds_n, then_none)           \
    {                                                                      \
        if ((sp) == 0) { (cur) = BVH4_NONE_W; then_none; }                 \
        (cur) = (uint32_t)BVH_POP(stack, sp, lds_slot, lds_n);             \
    }
// Same, culling: entries whose subtree starts at or beyond t are dropped.
#define BVH_POP_CLOSER(cur, stack, sp, lds_slot, lds_n, t, then_none, then_word) \
    for (;;) {                                                                   \
        if ((sp) == 0) { (cur) = BVH4_NONE_W; then_none; }                       \
        uint64_t e_ = BVH_POP(stack, sp, lds_slot, lds_n);                       \
        if (uint_as_float((uint32_t)(e_ >> 32)) < (t)) { (cur) = (uint32_t)e_; then_word; } \
    }

// Ordered visit of node nd: push the hit children far -> near (so the near
// ones pop first); next = the nearest one's word, BVH4_NONE_W if none is hit.
// (`next` is the caller's variable.)
#define BVH_VISIT_ORDERED(Node, next, nd, inv_d, o_div, tmax, stack, sp, lds_slot, lds_n) \
    BVH_HIT_KEYS(Node, nd, inv_d, o_div, tmax, keys_, nhit_)                           \
    next = BVH4_NONE_W;                                                                \
    for (int k_ = nhit_ - 1; k_ >= 0; --k_) {                                          \
        uint32_t lo_ = bvh_child_word_at(nd, keys_[k_] & (Node::WIDTH - 1u));          \
        if (lo_ == BVH4_NONE_W) continue; /* empty slot */                             \
        if (k_ == 0) {                                                                 \
            next = lo_;                                                                \
        } else {                                                                       \
            uint64_t e_ = ((uint64_t)(keys_[k_] & ~(Node::WIDTH - 1u)) << 32) | lo_;   \
            BVH_PUSH(stack, sp, lds_slot, lds_n, e_)                                   \
        }                                                                              \
    }

// The same visit for a width-4 node of tagged words (BVH4NodeT, BVH4NodeQ),
// without a run-time count or index: the device form.  Under wave64
// divergence every instruction of the visit costs a full issue slot however
// few lanes need it, so the form above is dear there: `keys[nhit++]` on a
// run-time nhit is a compare/select cascade per child, the sort sits in
// nested exec-masked blocks that a divergent wave enters nearly all of, and
// the push loop runs max(nhit) times per wave with a select tree per pass.
// Here a missed child gets the key BVH4_MISS_KEY, above every hit key (a
// hit key's top bit is clear: t_near >= 0), all four keys go through a fixed
// 5-comparator min/max network, and the three far keys are pushed far ->
// near in unrolled steps.  Hit keys are distinct (the slot is in the low
// bits), so any correct sort gives the order of the form above: `next` and
// every pushed entry are the same (tests/test_visit_host.py compares them).
//
// Each key travels through the network with its child's word, so nothing
// behind the sort has to find the word again from the slot bits (a select
// tree over the four words and a test for the miss key per push, and once
// more for `next`): a comparator is one compare on the keys and four selects.
// A missed child's word is BVH4_NONE_W, so misses need no order among
// themselves; a hit empty slot or leaf of no prims keeps its real key and has
// the word BVH4_NONE_W, which a push skips and which, as the nearest child,
// makes `next` BVH4_NONE_W: the walk pops.
constexpr uint32_t BVH4_MISS_KEY = 0xffffffffu;
#define BVH_KEY_MINMAX(a, b)                                              \
    {                                                                     \
        const uint32_t lo_ = (a) < (b) ? (a) : (b);                       \
        const uint32_t hi_ = (a) < (b) ? (b) : (a);                       \
        (a) = lo_; (b) = hi_;                                             \
    }
#define BVH_PAIR_MINMAX(ka, wa, kb, wb)                                   \
    {                                                                     \
        const bool lt_ = (ka) < (kb);                                     \
        const uint32_t klo_ = lt_ ? (ka) : (kb), khi_ = lt_ ? (kb) : (ka); \
        const uint32_t wlo_ = lt_ ? (wa) : (wb), whi_ = lt_ ? (wb) : (wa); \
        (ka) = klo_; (kb) = khi_; (wa) = wlo_; (wb) = whi_;               \
    }
#define BVH_PAIR4(key, word, nd, c, inv_d, o_div, tmax)                   \
    uint32_t key, word;                                                   \
    {                                                                     \
        float enter_, exit_;                                              \
        bvh_child_slab(nd, c, inv_d, o_div, tmax, enter_, exit_);         \
        const bool hit_ = !bvh_slot_known_empty(nd, c) && enter_ <= exit_; \
        key = hit_ ? (float_as_uint(enter_) & ~3u) | (uint32_t)(c) : BVH4_MISS_KEY; \
        word = hit_ ? bvh_filled_child_word(nd, c) : BVH4_NONE_W;         \
    }
#define BVH_PUSH_PAIR4(key, word, stack, sp, lds_slot, lds_n)             \
    {                                                                     \
        if ((word) != BVH4_NONE_W) {                                      \
            uint64_t e_ = ((uint64_t)((key) & ~3u) << 32) | (word);       \
            BVH_PUSH(stack, sp, lds_slot, lds_n, e_)                      \
        }                                                                 \
    }
#define BVH_VISIT_TAGGED4(next, nd, inv_d, o_div, tmax, stack, sp, lds_slot, lds_n) \
    BVH_PAIR4(k0_, w0_, nd, 0, inv_d, o_div, tmax)                        \
    BVH_PAIR4(k1_, w1_, nd, 1, inv_d, o_div, tmax)                        \
    BVH_PAIR4(k2_, w2_, nd, 2, inv_d, o_div, tmax)                        \
    BVH_PAIR4(k3_, w3_, nd, 3, inv_d, o_div, tmax)                        \
    BVH_PAIR_MINMAX(k0_, w0_, k1_, w1_)                                   \
    BVH_PAIR_MINMAX(k2_, w2_, k3_, w3_)                                   \
    BVH_PAIR_MINMAX(k0_, w0_, k2_, w2_)                                   \
    BVH_PAIR_MINMAX(k1_, w1_, k3_, w3_)                                   \
    BVH_PAIR_MINMAX(k1_, w1_, k2_, w2_)                                   \
    BVH_PUSH_PAIR4(k3_, w3_, stack, sp, lds_slot, lds_n)                  \
    BVH_PUSH_PAIR4(k2_, w2_, stack, sp, lds_slot, lds_n)                  \
    BVH_PUSH_PAIR4(k1_, w1_, stack, sp, lds_slot, lds_n)                  \
    next = w0_;
// The visit a walk over `Node` runs.
#define BVH_VISIT(Node, next, nd, inv_d, o_div, tmax, stack, sp, lds_slot, lds_n)      \
    if constexpr (Node::WIDTH == 4 && Node::TAGGED) {                                  \
        BVH_VISIT_TAGGED4(next, nd, inv_d, o_div, tmax, stack, sp, lds_slot, lds_n)    \
    } else {                                                                           \
        BVH_VISIT_ORDERED(Node, next, nd, inv_d, o_div, tmax, stack, sp, lds_slot, lds_n) \
    }

// Any-hit visit of node nd, one child after the other: the first hit child
// becomes next, the others are pushed as bare words.  next must come in as
// BVH4_NONE_W.  The visit the any-hit walk runs, and the other side of
// C.bvh4_any_visit_selftest.
#define BVH_VISIT_ANY_EACH(Node, next, nd, inv_d, o_div, tmax, stack, sp, lds_slot, lds_n) \
    _Pragma("unroll")                                                                  \
    for (int c_ = 0; c_ < Node::WIDTH; ++c_) {                                         \
        if (bvh_slot_known_empty(nd, c_)) continue;                                    \
        float enter_, exit_;                                                           \
        bvh_child_slab(nd, c_, inv_d, o_div, tmax, enter_, exit_);                     \
        if (enter_ > exit_) continue;                                                  \
        if constexpr (Node::TAGGED) {                                                  \
            /* the word says it (the quantized node's was looked at before its box) */ \
            if (!Node::EMPTY_BEFORE_BOX && nd.child[c_] == BVH4_NONE_W) continue;      \
        } else {                                                                       \
            /* the empty-slot rule, spelled out here: as the result of a helper the    \
               && compiles to different code */                                        \
            if (nd.child[c_] < 0 && nd.cnt[c_] == 0) continue;                         \
        }                                                                              \
        const uint32_t lo_ = bvh_filled_child_word(nd, c_);                            \
        if (next == BVH4_NONE_W) {                                                     \
            next = lo_;                                                                \
        } else {                                                                       \
            uint64_t e_ = (uint64_t)lo_;                                               \
            BVH_PUSH(stack, sp, lds_slot, lds_n, e_)                                   \
        }                                                                              \
    }

// The any-hit visit for a width-4 node of tagged words, in a straight line:
// a measured experiment that lost, kept host-tested behind BVH4_ANY_STRAIGHT.
// The any-hit walk returns a predicate — some prim of some reached leaf has
// EPSILON < t < tmax, tmax fixed for the whole walk — and does not cull on
// pop, so the order in which hit children are continued and pushed cannot
// change its result, and bare words are all it needs: no t_near key, no
// select tree.  Each child's value is its word if the box is hit, else a miss
// value; the four values go through the same 5-comparator min/max network as
// the keys of BVH_VISIT_TAGGED4, which compacts the hit words to the front;
// next is the first, the other three are pushed behind one test each.
// What BVH_VISIT_TAGGED4 gained over the ordered visit does not carry over:
// the form above has no key array, no sort and no push loop to lose, the
// compiler already turns it into three push sites, and a shadow ray misses
// most boxes, so its blocks are mostly skipped, while the network always
// runs.  gfx950 node phase of k_wf_shadow<4>: 205 -> 203 instructions;
// flagship 0.6% slower (profiles/README.md).
//
// The miss value and the comparison decide what comes first:
//   false: miss 0xffffffff, unsigned order: internal nodes, then leaves,
//          then misses — leaves are postponed, as the phase batching of the
//          while-while walk wants.  An empty slot's word (BVH4_NONE_W) lies
//          between nodes and leaves and is folded into the miss value.
//   true:  miss BVH4_NONE_W, signed order: leaves, then nodes, then misses
//          — prims are tested early, which favours the early exit.
// Leaves first measured another 0.6% slower than nodes first.
constexpr bool BVH4_ANY_STRAIGHT = false;
constexpr bool BVH4_ANY_LEAVES_FIRST = false;
constexpr uint32_t BVH4_ANY_MISS_W = BVH4_ANY_LEAVES_FIRST ? BVH4_NONE_W : 0xffffffffu;
// 0xffffffff is the word of a leaf of 15 prims at base 2^27-1.  No leaf has
// it as long as all prims lie below index BVH4_MAX_PRIMS (tag_bvh4 checks).
constexpr int BVH4_MAX_PRIMS = 0x07ffffff;
static_assert(BVH4_ANY_LEAVES_FIRST ||
              BVH4_ANY_MISS_W == (0x80000000u | (15u << 27) | (uint32_t)BVH4_MAX_PRIMS),
              "the any-hit miss value must be the one leaf word no tree holds");
#define BVH_ANY_WORD4(w, nd, c, inv_d, o_div, tmax)                       \
    uint32_t w;                                                           \
    {                                                                     \
        float enter_, exit_;                                              \
        bvh_child_slab(nd, c, inv_d, o_div, tmax, enter_, exit_);         \
        const bool hit_ = !bvh_slot_known_empty(nd, c) && enter_ <= exit_; \
        if constexpr (BVH4_ANY_LEAVES_FIRST)                              \
            w = hit_ ? nd.child[c] : BVH4_NONE_W;                         \
        else                                                              \
            w = hit_ && nd.child[c] != BVH4_NONE_W ? nd.child[c] : BVH4_ANY_MISS_W; \
    }
#define BVH_ANY_MINMAX(a, b)                                              \
    if constexpr (BVH4_ANY_LEAVES_FIRST) {                                \
        const uint32_t lo_ = (int32_t)(a) < (int32_t)(b) ? (a) : (b);     \
        const uint32_t hi_ = (int32_t)(a) < (int32_t)(b) ? (b) : (a);     \
        (a) = lo_; (b) = hi_;                                             \
    } else BVH_KEY_MINMAX(a, b)
#define BVH_PUSH_ANY4(w, stack, sp, lds_slot, lds_n)                      \
    if ((w) != BVH4_ANY_MISS_W) {                                         \
        uint64_t e_ = (uint64_t)(w);                                      \
        BVH_PUSH(stack, sp, lds_slot, lds_n, e_)                          \
    }
#define BVH_VISIT_ANY4(next, nd, inv_d, o_div, tmax, stack, sp, lds_slot, lds_n) \
    BVH_ANY_WORD4(w0_, nd, 0, inv_d, o_div, tmax)                         \
    BVH_ANY_WORD4(w1_, nd, 1, inv_d, o_div, tmax)                         \
    BVH_ANY_WORD4(w2_, nd, 2, inv_d, o_div, tmax)                         \
    BVH_ANY_WORD4(w3_, nd, 3, inv_d, o_div, tmax)                         \
    BVH_ANY_MINMAX(w0_, w1_)                                              \
    BVH_ANY_MINMAX(w2_, w3_)                                              \
    BVH_ANY_MINMAX(w0_, w2_)                                              \
    BVH_ANY_MINMAX(w1_, w3_)                                              \
    BVH_ANY_MINMAX(w1_, w2_)                                              \
    BVH_PUSH_ANY4(w3_, stack, sp, lds_slot, lds_n)                        \
    BVH_PUSH_ANY4(w2_, stack, sp, lds_slot, lds_n)                        \
    BVH_PUSH_ANY4(w1_, stack, sp, lds_slot, lds_n)                        \
    next = w0_ == BVH4_ANY_MISS_W ? BVH4_NONE_W : w0_;

// ------------------------------------------------------------- leaf loops
// Intersect prims [base, base+cnt) and tighten rec.  tri_only (a scene-
// uniform scalar) skips the per-prim prim_obj sphere-bit load entirely —
// the reference's TRIANGLE_ONLY compile flag ("10% faster", defines.cuh:
// 26-27) as a runtime-free SGPR branch.
//
// Both loops read the whole primitive into locals first (bvh_load_prim):
// three 16-byte loads issued together, with the sphere-bit load when there is
// one, and one wait for all of them.  Left to itself the compiler loads e1
// and e2, waits, tests det, and only behind that branch loads v0 and waits
// again: two dependent round trips per triangle, three with the sphere bit.
HD Prim bvh_load_prim(const Prim* prims, const uint32_t* prim_obj, int pid,
                      bool tri_only, bool& sph) {
    uint32_t obj = 0;
    if (!tri_only) obj = prim_obj[pid];
    const Prim p = prims[pid];
#if HIPPT_ON_DEVICE
    // An empty statement that reads all thirteen values: every load is
    // issued and has landed here, none can be narrowed or sunk behind the
    // det branch of intersect_triangle.  It emits no instruction.
    asm volatile("" :: "v"(obj), "v"(p.v0.x), "v"(p.v0.y), "v"(p.v0.z), "v"(p.v0.w),
                       "v"(p.e1.x), "v"(p.e1.y), "v"(p.e1.z), "v"(p.e1.w),
                       "v"(p.e2.x), "v"(p.e2.y), "v"(p.e2.z), "v"(p.e2.w));
#endif
    sph = (obj & PRIM_SPHERE_BIT) != 0;
    return p;
}
HD void bvh4_leaf_hit(const Prim* prims, const uint32_t* prim_obj,
                      const Ray& ray, int base, int cnt, HitRecord& rec,
                      bool tri_only = false) {
    for (int k = 0; k < cnt; ++k) {
        int pid = base + k;
        bool sph;
        const Prim p = bvh_load_prim(prims, prim_obj, pid, tri_only, sph);
        float u, v;
        float t = intersect_prim(p, sph, ray, u, v);
        if (t > EPSILON && t < rec.t) {
            rec.t = t; rec.u = u; rec.v = v; rec.prim_idx = pid;
        }
    }
}
// Any-hit form: `return true` from the walk if a prim of [base, base+cnt)
// blocks (EPSILON, tmax).  A macro because it leaves the walk from inside
// the loop.  tri_only as in bvh4_leaf_hit.
#define BVH_LEAF_ANY_RETURN(prims, prim_obj, ray, base, cnt, tmax, tri_only)  \
    for (int k_ = 0; k_ < (cnt); ++k_) {                                      \
        int pid_ = (base) + k_;                                               \
        bool sph_;                                                            \
        const Prim p_ = bvh_load_prim(prims, prim_obj, pid_, tri_only, sph_); \
        float u_, v_;                                                         \
        float t_ = intersect_prim(p_, sph_, ray, u_, v_);                     \
        if (t_ > EPSILON && t_ < (tmax)) return true;                         \
    }

// ------------------------------------------------------- LDS node cache
// Device kernels copy the first n_cached nodes of the traversal array into
// LDS (trav_lds.h); a walk reads node `cur` from that copy when cur <
// n_cached.  Which nodes those are is decided on the host: bvh4_top_first at
// the end of this file puts the nodes most rays visit first.
//
// Cached node i lives at byte i * TRAV_CACHE_STRIDE of the copy.  At the
// node's own 128 bytes, field f of node i falls on LDS banks 32*i + f/4 ..
// +3 (mod 64): all even nodes share one set of four banks and all odd nodes
// the other, so sixteen lanes on sixteen cached nodes are an 8-way conflict
// on each of the visit's 16-byte reads.  At 144 bytes node i starts on bank
// 36*i mod 64, and sixteen consecutive nodes cover the 64 banks once.
// Measured, the packed layout wins all the same: the padded one costs a
// select and a shift-add per visit and a stack entry of LDS per block, and
// the kitchen comes out 0.6-1.9 Msamples/s slower at every order and cache
// size (profiles/README.md).  HIPPT_CACHE_STRIDE=144 (setup.py) builds the
// padded layout for A/B runs.
#ifndef HIPPT_CACHE_STRIDE
#define HIPPT_CACHE_STRIDE 128
#endif
constexpr int TRAV_CACHE_STRIDE = HIPPT_CACHE_STRIDE;   // of the 128-byte node
static_assert(TRAV_CACHE_STRIDE >= 128 && TRAV_CACHE_STRIDE % 16 == 0,
              "cached nodes are read with 16-byte loads");
// The same padding behind a node of another size (the quantized node).
template <class Node>
constexpr int bvh_cache_stride() { return (int)sizeof(Node) + (TRAV_CACHE_STRIDE - 128); }
// Address of node cur: one address, one load sequence behind it.  The two
// strides differ by the padding only, so the offset is built in 16-byte
// units, cur * sizeof/16 plus cur * pad/16 when cached: a select and a
// shift-add more than the packed layout, no multiply and no second path.
// (A node index is below 2^27, so the units fit 32 bits.)
template <class Node>
HD const Node* bvh_node_at(const Node* nodes, const Node* top_cache, int n_cached,
                           uint32_t cur) {
    constexpr uint32_t PAD16 = (uint32_t)(bvh_cache_stride<Node>() - (int)sizeof(Node)) / 16u;
    const bool cached = (int)cur < n_cached;
    const Node* nsrc = cached ? top_cache : nodes;
    if constexpr (PAD16 == 0) {
        return nsrc + cur;
    } else {
        const uint32_t units = cur * (uint32_t)(sizeof(Node) / 16) + (cached ? cur * PAD16 : 0u);
        return (const Node*)((const char*)nsrc + (size_t)units * 16);
    }
}

// ------------------------------------------------------ while-while walks
// Aila & Laine style phase batching, re-derived for wave64: lanes alternate
// between a node-walk phase and a leaf-test phase at the OUTER loop level,
// so a wave tends to execute runs of same-kind work instead of interleaving
// a node step on some lanes with prim tests on others.  Leaf children are
// POSTPONED onto the stack (tagged entries) instead of intersected inline.
// Measured A/B against the inline walk (divergence: VALUUtilization 15% on
// the inline walk).
template <class Node>
HD HitRecord bvh_closest_ww(const Node* nodes, const Prim* prims,
                            const uint32_t* prim_obj, const Ray& ray, float tmax,
                            LdsSlot lds_slot, int lds_n, const Node* top_cache,
                            int n_cached, bool tri_only) {
    HitRecord rec;
    rec.t = tmax;
    const Vec3 inv_d = safe_rcp_dir(ray.d);
    const Vec3 o_div = ray.o * inv_d;
    uint64_t stack[BVH4_STACK];
    int sp = 0;
    uint32_t cur = 0;
    for (;;) {
        // ---- node phase: walk internal nodes until a leaf surfaces
        while (bvh4_is_node(cur)) {
            // the first n_cached nodes come from the LDS copy (top-first
            // order: the nodes most walks visit; LDS is ~4x closer than L2).
            // Address select, single flat load.
            const Node nd = *bvh_node_at(nodes, top_cache, n_cached, cur);
            uint32_t next;
            BVH_VISIT(Node, next, nd, inv_d, o_div, rec.t, stack, sp, lds_slot, lds_n)
            if (next != BVH4_NONE_W) { cur = next; continue; }
            BVH_POP_CLOSER(cur, stack, sp, lds_slot, lds_n, rec.t, break, break)
        }
        if (cur == BVH4_NONE_W) break;
        // ---- leaf phase: drain consecutive leaf entries
        while (bvh4_is_leaf(cur)) {
            bvh4_leaf_hit(prims, prim_obj, ray, bvh4_leaf_base(cur),
                          bvh4_leaf_count(cur), rec, tri_only);
            BVH_POP_CLOSER(cur, stack, sp, lds_slot, lds_n, rec.t, break, break)
        }
        if (cur == BVH4_NONE_W) break;
    }
    if (rec.prim_idx < 0) rec.t = MAX_DIST;
    return rec;
}
// Any-hit form: no ordering (any hit ends the walk), the first hit child
// continues and the others are pushed as bare words; `true` on the first
// blocking prim.  Measured +1-2% against the inline-leaf occlusion walk; now
// the default.
template <class Node>
HD bool bvh_any_ww(const Node* nodes, const Prim* prims, const uint32_t* prim_obj,
                   const Ray& ray, float tmax, LdsSlot lds_slot, int lds_n,
                   const Node* top_cache, int n_cached, bool tri_only) {
    const Vec3 inv_d = safe_rcp_dir(ray.d);
    const Vec3 o_div = ray.o * inv_d;
    uint64_t stack[BVH4_STACK];
    int sp = 0;
    uint32_t cur = 0;
    for (;;) {
        while (bvh4_is_node(cur)) {
            const Node nd = *bvh_node_at(nodes, top_cache, n_cached, cur);
            uint32_t next = BVH4_NONE_W;
            if constexpr (BVH4_ANY_STRAIGHT && Node::WIDTH == 4 && Node::TAGGED) {
                BVH_VISIT_ANY4(next, nd, inv_d, o_div, tmax, stack, sp, lds_slot, lds_n)
            } else {
                BVH_VISIT_ANY_EACH(Node, next, nd, inv_d, o_div, tmax, stack, sp, lds_slot, lds_n)
            }
            if (next != BVH4_NONE_W) { cur = next; continue; }
            BVH_POP_WORD(cur, stack, sp, lds_slot, lds_n, break)
        }
        if (cur == BVH4_NONE_W) return false;
        while (bvh4_is_leaf(cur)) {
            const int base = bvh4_leaf_base(cur), pc = bvh4_leaf_count(cur);
            BVH_LEAF_ANY_RETURN(prims, prim_obj, ray, base, pc, tmax, tri_only)
            BVH_POP_WORD(cur, stack, sp, lds_slot, lds_n, break)
        }
        if (cur == BVH4_NONE_W) return false;
    }
}

HD HitRecord ray_intersect_bvh4_ww(const BVH4NodeT* nodes,
                                   const Prim* prims, const uint32_t* prim_obj,
                                   const Ray& ray, float tmax,
                                   LdsSlot lds_slot = nullptr, int lds_n = 0,
                                   const BVH4NodeT* top_cache = nullptr,
                                   int n_cached = 0, bool tri_only = false) {
    return bvh_closest_ww(nodes, prims, prim_obj, ray, tmax, lds_slot, lds_n,
                          top_cache, n_cached, tri_only);
}
HD bool occlusion_test_bvh4_ww(const BVH4NodeT* nodes,
                               const Prim* prims, const uint32_t* prim_obj,
                               const Ray& ray, float tmax,
                               LdsSlot lds_slot = nullptr, int lds_n = 0,
                               const BVH4NodeT* top_cache = nullptr,
                               int n_cached = 0, bool tri_only = false) {
    return bvh_any_ww(nodes, prims, prim_obj, ray, tmax, lds_slot, lds_n,
                      top_cache, n_cached, tri_only);
}
// The same two walks over the quantized tree.
HD HitRecord ray_intersect_bvh4q_ww(const BVH4NodeQ* nodes,
                                    const Prim* prims, const uint32_t* prim_obj,
                                    const Ray& ray, float tmax,
                                    LdsSlot lds_slot = nullptr, int lds_n = 0,
                                    const BVH4NodeQ* top_cache = nullptr,
                                    int n_cached = 0) {
    return bvh_closest_ww(nodes, prims, prim_obj, ray, tmax, lds_slot, lds_n,
                          top_cache, n_cached, false);
}
HD bool occlusion_test_bvh4q_ww(const BVH4NodeQ* nodes,
                                const Prim* prims, const uint32_t* prim_obj,
                                const Ray& ray, float tmax,
                                LdsSlot lds_slot = nullptr, int lds_n = 0,
                                const BVH4NodeQ* top_cache = nullptr,
                                int n_cached = 0) {
    return bvh_any_ww(nodes, prims, prim_obj, ray, tmax, lds_slot, lds_n,
                      top_cache, n_cached, false);
}

// ------------------------------------------------------ inline-leaf walks
// Closest-hit ordered walk that intersects leaves inline, near -> far,
// tightening rec.t before far subtrees are entered: the walk the
// while-while form replaced on the device.  It shares the pieces but keeps a
// body of its own, as the independent side of bvh4_selftest.
HD HitRecord ray_intersect_bvh4(const BVH4Node* nodes,
                                const Prim* prims, const uint32_t* prim_obj,
                                const Ray& ray, float tmax = MAX_DIST,
                                LdsSlot lds_slot = nullptr, int lds_n = 0) {
    HitRecord rec;
    rec.t = tmax;
    const Vec3 inv_d = safe_rcp_dir(ray.d);
    const Vec3 o_div = ray.o * inv_d;
    uint64_t stack[BVH4_STACK];
    int sp = 0;
    uint32_t cur = 0;
    while (cur != BVH4_NONE_W) {
        const BVH4Node nd = nodes[cur];
        BVH_HIT_KEYS(BVH4Node, nd, inv_d, o_div, rec.t, keys, nhit)
        // internal children: the nearest continues, the rest are pushed
        cur = BVH4_NONE_W;
        for (int k = 0; k < nhit; ++k) {
            const uint32_t w = bvh_child_word_at(nd, keys[k] & 3u);
            if (w == BVH4_NONE_W) continue;
            if (bvh4_is_leaf(w)) {
                bvh4_leaf_hit(prims, prim_obj, ray, bvh4_leaf_base(w), bvh4_leaf_count(w), rec);
            } else if (cur == BVH4_NONE_W) {
                cur = w;
            } else {
                uint64_t e = ((uint64_t)(keys[k] & ~3u) << 32) | w;
                BVH_PUSH(stack, sp, lds_slot, lds_n, e)
            }
        }
        if (cur == BVH4_NONE_W) BVH_POP_CLOSER(cur, stack, sp, lds_slot, lds_n, rec.t, break, break)
    }
    if (rec.prim_idx < 0) rec.t = MAX_DIST;
    return rec;
}

// Any-hit occlusion test with inline leaves: true if something blocks
// (EPSILON, tmax).  Unordered; only node indices are stacked.  One body for
// widths 4 and 8.
template <int W>
HD bool bvh_any_inline(const BVHWideNode<W>* nodes, const Prim* prims,
                       const uint32_t* prim_obj, const Ray& ray, float tmax,
                       LdsSlot lds_slot, int lds_n) {
    const Vec3 inv_d = safe_rcp_dir(ray.d);
    const Vec3 o_div = ray.o * inv_d;
    uint64_t stack[BVH4_STACK];
    int sp = 0;
    uint32_t cur = 0;
    while (cur != BVH4_NONE_W) {
        const BVHWideNode<W> nd = nodes[cur];
        cur = BVH4_NONE_W;
#pragma unroll
        for (int c = 0; c < W; ++c) {
            float enter, exit_;
            bvh_child_slab(nd, c, inv_d, o_div, tmax, enter, exit_);
            if (enter > exit_) continue;
            const int ch = nd.child[c];
            if (ch < 0) {
                const int base = ~ch, pc = nd.cnt[c];
                BVH_LEAF_ANY_RETURN(prims, prim_obj, ray, base, pc, tmax, false)
            } else if (cur == BVH4_NONE_W) {
                cur = (uint32_t)ch;
            } else {
                BVH_PUSH(stack, sp, lds_slot, lds_n, (uint64_t)(uint32_t)ch)
            }
        }
        if (cur == BVH4_NONE_W) BVH_POP_WORD(cur, stack, sp, lds_slot, lds_n, break)
    }
    return false;
}
HD bool occlusion_test_bvh4(const BVH4Node* nodes,
                            const Prim* prims, const uint32_t* prim_obj,
                            const Ray& ray, float tmax,
                            LdsSlot lds_slot = nullptr, int lds_n = 0) {
    return bvh_any_inline(nodes, prims, prim_obj, ray, tmax, lds_slot, lds_n);
}

// Node-visit / prim-test counting walk for the BVH-cost visualizer
// (reference pt_impl/bvh_cost.cu:38-101; counts reflect the traversal that
// actually runs, i.e. the 4-wide tree).  Unordered, inline leaves, boxes
// culled against the best t so far; the stack is private only.
HD Vec2 bvh4_cost(const BVH4Node* nodes, const Prim* prims,
                  const uint32_t* prim_obj, const Ray& ray) {
    const Vec3 inv_d = safe_rcp_dir(ray.d);
    const Vec3 o_div = ray.o * inv_d;
    HitRecord rec;
    rec.t = MAX_DIST;
    int node_visits = 0, prim_tests = 0;
    uint32_t stack[BVH4_STACK];
    const LdsSlot no_lds = nullptr;
    int sp = 0;
    uint32_t cur = 0;
    while (cur != BVH4_NONE_W) {
        const BVH4Node nd = nodes[cur];
        ++node_visits;
        cur = BVH4_NONE_W;
        for (int c = 0; c < 4; ++c) {
            float enter, exit_;
            bvh_child_slab(nd, c, inv_d, o_div, rec.t, enter, exit_);
            if (enter > exit_) continue;
            const int ch = nd.child[c];
            if (ch < 0) {
                prim_tests += nd.cnt[c];
                bvh4_leaf_hit(prims, prim_obj, ray, ~ch, nd.cnt[c], rec);
            } else if (cur == BVH4_NONE_W) {
                cur = (uint32_t)ch;
            } else {
                BVH_PUSH(stack, sp, no_lds, 0, (uint32_t)ch)
            }
        }
        if (cur == BVH4_NONE_W) BVH_POP_WORD(cur, stack, sp, no_lds, 0, break)
    }
    return {(float)node_visits, (float)prim_tests};
}

// -------------------------------------------------------------- dual walk
// One thread advances TWO independent closest-hit while-while walks in
// lockstep steps, so each lane keeps two node loads in flight (the
// single-ray walk stalls ~58% on L2-hit latency; a second independent chain
// per lane doubles memory-level parallelism without needing more waves).
// Used by the wavefront trace kernel (HIPPT_WF_DUAL).  Each walk gets half
// of the thread's LDS stack slots.
struct Bvh4Walk {
    HitRecord rec;
    uint32_t cur;       // tagged word; BVH4_NONE_W = finished
    int sp;
    Vec3 inv_d, o_div;
    Ray ray;
    uint64_t stack[BVH4_STACK / 2];
};

HD void bvh4_walk_init(Bvh4Walk& w, const Ray& ray, float tmax) {
    w.rec = HitRecord();
    w.rec.t = tmax;
    w.cur = 0;
    w.sp = 0;
    w.inv_d = safe_rcp_dir(ray.d);
    w.o_div = ray.o * w.inv_d;
    w.ray = ray;
}

// One step: a node visit (test 4 children, descend/push) OR one leaf batch.
// Returns true while the walk still has work.
HD bool bvh4_walk_step(Bvh4Walk& w, const BVH4NodeT* nodes, const Prim* prims,
                       const uint32_t* prim_obj, LdsSlot lds_slot, int lds_n) {
    if (w.cur == BVH4_NONE_W) return false;
    if (bvh4_not_leaf(w.cur)) {
        const BVH4NodeT nd = nodes[w.cur];
        uint32_t next;
        BVH_VISIT_TAGGED4(next, nd, w.inv_d, w.o_div, w.rec.t,
                          w.stack, w.sp, lds_slot, lds_n)
        if (next != BVH4_NONE_W) { w.cur = next; return true; }
    } else {
        bvh4_leaf_hit(prims, prim_obj, w.ray, bvh4_leaf_base(w.cur),
                      bvh4_leaf_count(w.cur), w.rec);
    }
    BVH_POP_CLOSER(w.cur, w.stack, w.sp, lds_slot, lds_n, w.rec.t, return false, return true)
}

// Host-side conversion BVH4Node -> traversal node: boxes copied, every slot's
// word tagged once here instead of on every visit.
inline std::vector<BVH4NodeT> tag_bvh4(const BVH4Node* nodes, int n) {
    std::vector<BVH4NodeT> out((size_t)(n > 0 ? n : 0));
    for (int i = 0; i < n; ++i) {
        const BVH4Node& s = nodes[i];
        BVH4NodeT& t = out[i];
        std::memcpy(t.lo_x, s.lo_x, 6 * 4 * sizeof(float));
        for (int c = 0; c < 4; ++c) {
            // prims below BVH4_MAX_PRIMS: the base fits its 27 bits and no
            // leaf word is the any-hit visit's miss value
            if (s.child[c] < 0 && (int64_t)(~s.child[c]) + s.cnt[c] > BVH4_MAX_PRIMS)
                throw std::runtime_error("tag_bvh4: leaf beyond BVH4_MAX_PRIMS prims");
            t.child[c] = bvh4_child_word(s.child[c], s.cnt[c]);
            t.pad[c] = 0;
        }
    }
    return out;
}

// Host-side node order for the traversal mirrors: the nodes most walks visit
// first, so that the LDS node cache (the first n_cached nodes, whatever
// n_cached a launch is granted) holds the tree's top.  collapse_bvh4 numbers
// nodes depth-first: its first 64 are the root, one node per level down the
// leftmost spine and one corner of the scene.
//   * The root stays node 0.
//   * Positions 1 .. min(n, n_top)-1 are filled one at a time from the open
//     set, the not yet placed internal children of the nodes placed so far,
//     with the open node of the highest priority; ties go to the lower source
//     index.  So every prefix is closed under "parent", and one order serves
//     every cache size.
//       TOP_AREA   priority = surface area of the node's box in its parent's
//                  slot, computed in double (a ray's chance to reach it)
//       TOP_LEVEL  priority = -depth (breadth first)
//       TOP_DFS    the input order, untouched
//   * All other nodes follow in their source order: deep subtrees stay
//     contiguous.
// Internal child indices are renumbered; boxes, leaf words, counts and the
// slot order are copied untouched, so a walk visits the same boxes and prims
// in the same order and only the node indices it carries differ.
// perm[source index] = new index.
constexpr int BVH4_TOP_ORDERED = 512;   // above the largest cache lds_plan grants
enum BVH4TopOrder { TOP_DFS = 0, TOP_LEVEL = 1, TOP_AREA = 2 };
constexpr BVH4TopOrder BVH4_TOP_ORDER_DEFAULT = TOP_AREA;   // HIPPT_TOP_ORDER overrides
inline std::vector<BVH4Node> bvh4_top_first(const BVH4Node* nodes, int n, int n_top,
                                            BVH4TopOrder order, std::vector<int32_t>& perm) {
    if (n < 0) n = 0;
    perm.resize((size_t)n);
    for (int i = 0; i < n; ++i) perm[i] = i;
    std::vector<BVH4Node> out(nodes, nodes + n);
    const int k_top = n_top < n ? n_top : n;
    if (order == TOP_DFS || k_top <= 1) return out;
    for (int i = 0; i < n; ++i)
        for (int c = 0; c < 4; ++c)
            if (nodes[i].child[c] >= n)
                throw std::runtime_error("bvh4_top_first: child index beyond the node array");
    struct Open { double prio; int node; };
    struct Later {   // a comes out of the queue after b
        bool operator()(const Open& a, const Open& b) const {
            return a.prio < b.prio || (a.prio == b.prio && a.node > b.node);
        }
    };
    std::priority_queue<Open, std::vector<Open>, Later> open;
    std::vector<int> depth((size_t)n, 0);
    std::vector<char> placed((size_t)n, 0);
    std::vector<int> src;   // src[new index] = source index
    src.reserve((size_t)n);
    auto place = [&](int i) {
        placed[i] = 1;
        src.push_back(i);
        const BVH4Node& s = nodes[i];
        for (int c = 0; c < 4; ++c) {
            const int ch = s.child[c];
            if (ch < 0 || placed[ch]) continue;
            depth[ch] = depth[i] + 1;
            double prio = -(double)depth[ch];
            if (order == TOP_AREA) {
                const double dx = (double)s.hi_x[c] - (double)s.lo_x[c];
                const double dy = (double)s.hi_y[c] - (double)s.lo_y[c];
                const double dz = (double)s.hi_z[c] - (double)s.lo_z[c];
                prio = 2.0 * (dx * dy + dy * dz + dz * dx);
                if (!(prio >= 0.0)) prio = 0.0;   // inverted or NaN box
            }
            open.push({prio, ch});
        }
    };
    place(0);
    while ((int)src.size() < k_top && !open.empty()) {
        const int i = open.top().node;
        open.pop();
        if (!placed[i]) place(i);
    }
    for (int i = 0; i < n; ++i)
        if (!placed[i]) src.push_back(i);
    for (int k = 0; k < n; ++k) perm[src[k]] = k;
    for (int k = 0; k < n; ++k) {
        out[k] = nodes[src[k]];
        for (int c = 0; c < 4; ++c)
            if (out[k].child[c] >= 0) out[k].child[c] = perm[out[k].child[c]];
    }
    return out;
}

// Host-side conversion fp32 4-wide -> quantized (outward rounding).
inline std::vector<BVH4NodeQ> quantize_bvh4(const BVH4Node* nodes, int n) {
    std::vector<BVH4NodeQ> out((size_t)n);
    for (int i = 0; i < n; ++i) {
        const BVH4Node& s = nodes[i];
        BVH4NodeQ& q = out[i];
        // node box = union of child boxes
        float lo[3] = {3e38f, 3e38f, 3e38f}, hi[3] = {-3e38f, -3e38f, -3e38f};
        for (int c = 0; c < 4; ++c) {
            if (s.child[c] == 0 && s.cnt[c] == 0) continue;  // empty
            lo[0] = fminf(lo[0], s.lo_x[c]); hi[0] = fmaxf(hi[0], s.hi_x[c]);
            lo[1] = fminf(lo[1], s.lo_y[c]); hi[1] = fmaxf(hi[1], s.hi_y[c]);
            lo[2] = fminf(lo[2], s.lo_z[c]); hi[2] = fmaxf(hi[2], s.hi_z[c]);
        }
        if (lo[0] > hi[0]) { lo[0] = lo[1] = lo[2] = 0.f; hi[0] = hi[1] = hi[2] = 0.f; }
        q.ox = lo[0]; q.oy = lo[1]; q.oz = lo[2];
        uint8_t* eptr = &q.ex;
        for (int a = 0; a < 3; ++a) {
            float ext = fmaxf(hi[a] - lo[a], 0.f);
            // smallest power-of-two scale with 255*scale >= ext
            int e = 127;  // scale 1 -> covers ext <= 255
            if (ext > 0.f) {
                float need = ext / 255.f;
                int ee;
                frexpf(need, &ee);         // need = m * 2^ee, m in [0.5,1)
                e = 127 + ee;              // 2^ee >= need
                if (e < 1) e = 1;
                if (e > 254) e = 254;
            }
            eptr[a] = (uint8_t)e;
        }
        q.pad = 0;
        const float sxyz[3] = {bvh4q_scale(q.ex), bvh4q_scale(q.ey), bvh4q_scale(q.ez)};
        for (int c = 0; c < 4; ++c) {
            if (s.child[c] == 0 && s.cnt[c] == 0) {
                q.child[c] = BVH4_NONE_W;
                for (int a = 0; a < 3; ++a) { q.qlo[c][a] = 255; q.qhi[c][a] = 0; }
                continue;
            }
            const float clo[3] = {s.lo_x[c], s.lo_y[c], s.lo_z[c]};
            const float chi[3] = {s.hi_x[c], s.hi_y[c], s.hi_z[c]};
            for (int a = 0; a < 3; ++a) {
                float inv_s = 1.f / sxyz[a];
                float fl = floorf((clo[a] - (&q.ox)[a]) * inv_s);
                float fh = ceilf((chi[a] - (&q.ox)[a]) * inv_s);
                q.qlo[c][a] = (uint8_t)clampv((int)fl, 0, 255);
                q.qhi[c][a] = (uint8_t)clampv((int)fh, 0, 255);
            }
            q.child[c] = bvh4_child_word(s.child[c], s.cnt[c]);
        }
    }
    return out;
}

} // namespace hippt
