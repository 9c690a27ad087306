// shade_load.h — the per-primitive shade word and the whole-record loaders
// of the shading code between the walks.
//
// Shading is bound by dependent-load latency like the walks are.  Read through
// references, a hit's inputs arrive one field at a time, each load behind a
// wait of its own and many of them behind a branch: prim_obj -> objs ->
// bsdfs -> tex[] was four round trips before the first BSDF field landed.
// The loaders here copy a record by value and then name every loaded dword
// in an empty asm statement (the bvh_load_prim pattern, bvh4.h): the loads
// are issued together, land behind one wait, and can be neither narrowed to
// the fields a branch happens to read nor sunk behind that branch.
//
// The host compiles the same functions without the statement, and hands out
// a reference into the table where the device hands out a copy: the CPU
// renderer is the bit-level reference of the goldens, and under -ffast-math
// a by-value record moves its loads to another block, which is enough for
// the host optimizer to associate a product chain in another order (one
// pixel of tests/golden/hero.npz, measured).  Callers therefore bind the
// result as `const auto&`, which is the table entry on the host and the
// lifetime-extended copy on the device.
//
// Callers read `tex[slot]` of a by-value BsdfParams with constant slots
// only: a run-time index would turn the copy into a private-memory slot
// (docs/TUNING.md, ScratchSize).
#pragma once
#include "geometry.h"
#include "bsdf.h"
#include "emitter.h"

namespace hippt {

// ---------------------------------------------------------------- shade word
// One uint32 per primitive, in BVH order, built on the host from prim_obj and
// objs (build_prim_shade below): what a hit needs of its object without the
// prim_obj -> objs hop.  The BSDF *type* is not in the word: update_bsdf
// changes it on a live scene.  Media ids stay in ObjInfo.
//   bit 31      sphere bit (same place as PRIM_SPHERE_BIT)
//   bits 16-30  emitter_id + 1, 0 = not an emitter
//   bits 0-15   bsdf_id
constexpr uint32_t SHADE_BSDF_MASK = 0xFFFFu;
constexpr uint32_t SHADE_EMITTER_MASK = 0x7FFFu;
constexpr int SHADE_EMITTER_SHIFT = 16;
constexpr int SHADE_MAX_BSDFS = 65536;
constexpr int SHADE_MAX_EMITTERS = 32767;

HD int shade_bsdf_id(uint32_t w) { return (int)(w & SHADE_BSDF_MASK); }
HD int shade_emitter_id(uint32_t w) {
    return (int)((w >> SHADE_EMITTER_SHIFT) & SHADE_EMITTER_MASK) - 1;
}
HD bool shade_is_sphere(uint32_t w) { return (w & PRIM_SPHERE_BIT) != 0; }

// objs is the (n_objs, 8) int32 table behind ObjInfo; only bsdf_id and
// emitter_id are read.  Returns false (and the offending primitive) when an
// id does not fit its field.
inline bool build_prim_shade(const uint32_t* prim_obj, int n_prims,
                             const int32_t* objs, int n_objs,
                             uint32_t* out, int* bad_prim) {
    for (int i = 0; i < n_prims; ++i) {
        const uint32_t oi = prim_obj[i] & PRIM_OBJ_MASK;
        if ((int)oi >= n_objs) { if (bad_prim) *bad_prim = i; return false; }
        const int32_t bsdf_id = objs[oi * 8 + 2];
        const int32_t emitter_id = objs[oi * 8 + 3];
        if (bsdf_id < 0 || bsdf_id >= SHADE_MAX_BSDFS || emitter_id >= SHADE_MAX_EMITTERS) {
            if (bad_prim) *bad_prim = i;
            return false;
        }
        const uint32_t em = emitter_id >= 0 ? (uint32_t)(emitter_id + 1) : 0u;
        out[i] = (prim_obj[i] & PRIM_SPHERE_BIT) | (em << SHADE_EMITTER_SHIFT) |
                 (uint32_t)bsdf_id;
    }
    return true;
}

// ------------------------------------------------------------------- loaders
#if HIPPT_ON_DEVICE
#define HIPPT_LANDED_EMITTER(e)                                             \
    HIPPT_LANDED_VEC4((e).emission), HIPPT_LANDED_VEC4((e).aux),            \
    "v"((e).type), "v"((e).obj_id), "v"((e).tex_id), "v"((e).prim_base),    \
    "v"((e).prim_cnt), "v"((e).inv_area), "v"((e).extra0), "v"((e).extra1)
#endif

// Group 1 of a hit: the 64-byte attribute record and the shade word.
// HitShade (and EmitterPick, scene_view.h) has a reference member on the host
// and a value member on the device, so its layout differs between the two
// passes of one translation unit: it is a function-local temporary only, and
// must never be stored, put into a buffer or passed to a kernel.
#if !HIPPT_ON_DEVICE
struct HitShade {
    const PrimAttr& attr;
    uint32_t word;
};
template <class SV>
HD HitShade load_hit_shade(const SV& sv, int prim_idx) {
    return {sv.attrs[prim_idx], sv.prim_shade[prim_idx]};
}
#else
struct HitShade {
    PrimAttr attr;
    uint32_t word;
};
template <class SV>
HD HitShade load_hit_shade(const SV& sv, int prim_idx) {
    HitShade h;
    h.word = sv.prim_shade[prim_idx];
    h.attr = sv.attrs[prim_idx];
    asm volatile("" :: "v"(h.word), HIPPT_LANDED_VEC4(h.attr.n0), HIPPT_LANDED_VEC4(h.attr.n1),
                       HIPPT_LANDED_VEC4(h.attr.n2), HIPPT_LANDED_VEC4(h.attr.uvrest));
    return h;
}
#endif

// The 80-byte BSDF record, tex[] as four packed dwords.
#if !HIPPT_ON_DEVICE
HD const BsdfParams& load_bsdf(const BsdfParams* bsdfs, int id) { return bsdfs[id]; }
HD const EmitterParams& load_emitter(const EmitterParams* emitters, int i) { return emitters[i]; }
#else
HD BsdfParams load_bsdf(const BsdfParams* bsdfs, int id) {
    const BsdfParams b = bsdfs[id];
    uint32_t t0, t1, t2, t3;
    __builtin_memcpy(&t0, &b.tex[0], 4);
    __builtin_memcpy(&t1, &b.tex[2], 4);
    __builtin_memcpy(&t2, &b.tex[4], 4);
    __builtin_memcpy(&t3, &b.tex[6], 4);
    asm volatile("" :: HIPPT_LANDED_VEC4(b.kd), HIPPT_LANDED_VEC4(b.ks), HIPPT_LANDED_VEC4(b.kg),
                       "v"(b.type), "v"(b.ior), "v"(b.extra0), "v"(b.extra1),
                       "v"(t0), "v"(t1), "v"(t2), "v"(t3));
    return b;
}

// The 64-byte emitter record.
HD EmitterParams load_emitter(const EmitterParams* emitters, int i) {
    const EmitterParams e = emitters[i];
    asm volatile("" :: HIPPT_LANDED_EMITTER(e));
    return e;
}
#endif

// The emitter record together with the two selection-CDF words of its pick
// pdf (cdf[i] - cdf[i-1], the expression of emitter_sel_pdf), behind one wait.
#if !HIPPT_ON_DEVICE
HD const EmitterParams& load_emitter_sel(const EmitterParams* emitters, const float* sel_cdf,
                                         int i, float& pdf) {
    pdf = sel_cdf[i] - (i ? sel_cdf[i - 1] : 0.f);
    return emitters[i];
}
#else
HD EmitterParams load_emitter_sel(const EmitterParams* emitters, const float* sel_cdf,
                                  int i, float& pdf) {
    const float hi = sel_cdf[i];
    const float lo = sel_cdf[i ? i - 1 : 0];
    const EmitterParams e = emitters[i];
    asm volatile("" :: "v"(hi), "v"(lo), HIPPT_LANDED_EMITTER(e));
    pdf = hi - (i ? lo : 0.f);
    return e;
}
#undef HIPPT_LANDED_EMITTER
#endif

// ------------------------------------------------------------------- probe
// The raw records a hit gathers, as dwords in memory order, through the
// loaders above: 16 attribute words, the shade word, 20 BSDF words, 16
// emitter words (zeros when the primitive is not an emitter).  Host and
// device run this same body (Scene.shade_probe, k_shade_probe).  Ids that
// point outside their table leave zeros instead of reading there.
constexpr int SHADE_PROBE_WORDS = 16 + 1 + 20 + 16;

HD void shade_probe_vec4(uint32_t* out, const Vec4& v) {
    out[0] = float_as_uint(v.x); out[1] = float_as_uint(v.y);
    out[2] = float_as_uint(v.z); out[3] = float_as_uint(v.w);
}
HD uint32_t shade_probe_tex2(int16_t lo, int16_t hi) {
    return (uint32_t)(uint16_t)lo | ((uint32_t)(uint16_t)hi << 16);
}
template <class SV>
HD void shade_probe_record(const SV& sv, int prim_idx, uint32_t* out) {
    for (int k = 0; k < SHADE_PROBE_WORDS; ++k) out[k] = 0u;
    const HitShade hs = load_hit_shade(sv, prim_idx);
    shade_probe_vec4(out + 0, hs.attr.n0);
    shade_probe_vec4(out + 4, hs.attr.n1);
    shade_probe_vec4(out + 8, hs.attr.n2);
    shade_probe_vec4(out + 12, hs.attr.uvrest);
    out[16] = hs.word;
    const int bsdf_id = shade_bsdf_id(hs.word);
    if (bsdf_id < sv.n_bsdfs) {
        const auto& b = load_bsdf(sv.bsdfs, bsdf_id);
        shade_probe_vec4(out + 17, b.kd);
        shade_probe_vec4(out + 21, b.ks);
        shade_probe_vec4(out + 25, b.kg);
        out[29] = (uint32_t)b.type;
        out[30] = float_as_uint(b.ior);
        out[31] = float_as_uint(b.extra0);
        out[32] = float_as_uint(b.extra1);
        out[33] = shade_probe_tex2(b.tex[0], b.tex[1]);
        out[34] = shade_probe_tex2(b.tex[2], b.tex[3]);
        out[35] = shade_probe_tex2(b.tex[4], b.tex[5]);
        out[36] = shade_probe_tex2(b.tex[6], b.tex[7]);
    }
    const int emitter_id = shade_emitter_id(hs.word);
    if (emitter_id >= 0 && emitter_id < sv.n_emitters) {
        const auto& e = load_emitter(sv.emitters, emitter_id);
        shade_probe_vec4(out + 37, e.emission);
        shade_probe_vec4(out + 41, e.aux);
        out[45] = (uint32_t)e.type;
        out[46] = (uint32_t)e.obj_id;
        out[47] = (uint32_t)e.tex_id;
        out[48] = (uint32_t)e.prim_base;
        out[49] = (uint32_t)e.prim_cnt;
        out[50] = float_as_uint(e.inv_area);
        out[51] = float_as_uint(e.extra0);
        out[52] = float_as_uint(e.extra1);
    }
}

} // namespace hippt
