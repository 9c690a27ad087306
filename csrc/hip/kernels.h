// kernels.h — launch API of the gfx950 HIP kernels (implemented in *.hip).
#pragma once
#include <cstdint>
#include "../core/scene_view.h"

namespace hippt {

enum RendererKind : int {
    R_MEGAKERNEL_PT = 0,
    R_WAVEFRONT_PT = 1,
    R_VOLUME_PT = 2,
    R_LIGHT_TRACE = 3,
    R_DEPTH = 4,
    R_BVH_COST = 5,
    R_MEGAKERNEL_PT_DYN = 6,
};

// Accumulate nspp samples into accum (h*w*4: RGB sum + count) and var
// (h*w*2: lum sum, lum^2 sum). sv must hold DEVICE pointers.
// Returns hipError_t as int.
// y0/y1: optional row band [y0, y1) for tile-split DP (0,0 = full frame);
// applies to the megakernel renderers (wavefront/lt always render full).
// spp_map: optional per-pixel sample budget for this launch (adaptive
// sampling; overrides nspp per pixel, 0 = skip pixel).
int launch_render(const SceneView& sv, float* accum, float* var,
                  int spp0, int nspp, uint32_t seed, int renderer,
                  int spec_constraint, float caustic_scaling,
                  void* stream, int y0 = 0, int y1 = 0,
                  const uint8_t* spp_map = nullptr,
                  float* aux = nullptr);  // (h*w*8) primary-hit AOV sums:
                                          // n.xyz, depth, albedo.rgb, count

// Wavefront path tracer (SoA queues + compaction); state owned by WfState.
struct WfState;
// payload (pixel) ids ride in the low 24 bits of every sort entry
constexpr int WF_MAX_PIXELS = 1 << 24;
WfState* wf_create(int width, int height);   // null above WF_MAX_PIXELS pixels
void wf_destroy(WfState* s);
int launch_render_wavefront(WfState* st, const SceneView& sv, float* accum, float* var,
                            int spp0, int nspp, uint32_t seed, int sort_mode, void* stream);

// Test probes (host pointers in and out; tests/test_gpu_probe.py).
// wf_sort_probe runs the renderer's sort pass once: over status[0..n), or
// over status[gather[k] & 0xFFFFFF], k in [0, m), when m > 0.  out[n] is
// pre-filled with 0xFFFFFFFF; the live entries land in out[0..*live).
int wf_sort_probe(const uint32_t* status, int n, const uint32_t* gather, int m,
                  int mode, uint32_t* out, int* live);
// wf_trace_probe runs scene_intersect + scene_occluded for n rays (ray_o_tmax:
// n x (ox, oy, oz, tmax); ray_d: n x (dx, dy, dz, -)) in the production LDS
// layout.  lds_n / n_cached < 0 take the render launcher's own values;
// explicit ones pass through the launcher's clamps.  hit_out: n x (t, u, v,
// prim as int bits); occ_out: n; plan_out: the (lds_n, n_cached) used.
int wf_trace_probe(const SceneView& sv, const float* ray_o_tmax, const float* ray_d,
                   int n, int lds_n, int n_cached, float* hit_out, int* occ_out,
                   int* plan_out);
// shade_probe runs shade_probe_record (core/shade_load.h) for n primitive
// indices, each already checked against sv.n_prims by the caller; out: n x
// SHADE_PROBE_WORDS dwords.
int shade_probe(const SceneView& sv, const int* prim_idx, int n, uint32_t* out);

// device helpers used by bind.cpp
int dev_malloc(void** p, size_t n);
int dev_free(void* p);
int dev_upload(void* dst, const void* src, size_t n);
int dev_memset(void* dst, int v, size_t n, void* stream);
int dev_synchronize();
int dev_set_device(int d);

} // namespace hippt
