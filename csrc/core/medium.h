// medium.h — participating media: homogeneous (analytic, 3-channel MIS) and
// density grids (delta-tracking distance sampling, ratio-tracking
// transmittance, blackbody emission from a temperature grid).
//
// Capability parity: reference src/core/medium.cuh, volume/homogeneous.cuh
// (per-RGB-channel MIS distance sampling with the numerically-stable
// 3-channel weighting, homogeneous.cuh:43-83), volume/grid.cuh +
// impl/vol_grid.cu (NanoVDB delta tracking :128-150, ratio tracking with RR
// at Tr<0.1 :177-198, residual-ratio variant :153-175, stochastic-offset
// nearest-neighbor lookup, blackbody emission :97-102).
//
// MI355X-native change: instead of walking NanoVDB trees on-device (long
// scalar-dependent pointer chases) the voxels live in a flat device buffer
// plus a majorant SUPERGRID that delta/ratio tracking DDA over.  Two voxel
// layouts share every line of the tracking code:
//   dense  — one (nz,ny,nx) float array (default; every shipped grid),
//   bricks — a brick table over ceil(n/8) cells per axis holding a pool
//            index or -1, plus a pool of resident 8^3 bricks (512 floats
//            each): two dependent loads per lookup, no dense expansion of
//            large mostly-empty volumes (hippt/scene/sparse_grid.py).
// The host layer loads grids from .npy / .nvdb files (hippt/scene/nvdb.py)
// or procedural generators.
#pragma once
#include "phase.h"
#include "spectrum.h"

namespace hippt {

enum MediumType : int {
    MED_HOMOGENEOUS = 0,
    MED_GRID,
};

struct alignas(16) MediumParams {
    Vec4 sigma_a;          // absorption (homogeneous) / albedo-scaled (grid)
    Vec4 sigma_s;          // scattering
    Vec4 grid_lo;          // world-space grid bounds
    Vec4 grid_inv_extent;  // 1 / (hi - lo)
    const float* density;      // nx*ny*nz density voxels (nullptr for homogeneous);
                               // brick pool (512 floats/brick) when `bricks` is set
    const float* temperature;  // optional emission temperature grid (same layout)
    // majorant supergrid: per-supercell RAW density max (HIPPT_SUPER_N
    // voxels/cell per axis, default 16; dilated by 1 voxel for the
    // stochastic-offset lookup); the tracking
    // walks DDA over it so null collisions never happen in empty space
    // (reference uses one global majorant from tree extrema, vol_grid.cu:131)
    const float* super;
    // brick layout: bnx*bny*bnz table of pool indices (-1 = empty brick,
    // background 0); nullptr = dense layout
    const int32_t* bricks;
    int32_t sx, sy, sz;
    int32_t nx, ny, nz;
    int32_t bnx, bny, bnz;
    int32_t type;
    int32_t phase_id;
    float majorant;        // max sigma_t over the grid (delta tracking)
    float avg_density;     // mean density (residual-ratio control)
    float scale;           // density multiplier
    float emission_scale;  // blackbody emission brightness
    float temp_scale;      // temperature units -> Kelvin
};
static_assert(sizeof(MediumParams) % 16 == 0, "MediumParams must stay 16-byte granular");

struct MediumSample {
    Vec3 local_thp;   // throughput multiplier up to the event
    float dist;       // distance of the scatter event (valid if scattered)
    bool scattered;   // true = real scatter event inside the medium
};

// ---------------------------------------------------------------- density
// Raw voxel fetch for either layout.  Both branches only LOAD; the caller
// applies any arithmetic after the merge, so the two layouts feed identical
// values into identical instructions (bit-equal renders).
//
// BRICKS (here and on every function down from trace_path_volumetric) says
// whether the scene may hold brick media at all.  The vpt kernel is built
// once per value: a scene without brick media runs the BRICKS=false
// instantiation, whose tracking loops carry no layout test, no extra live
// registers and no brick code (the shared kernel cost the dense smoke bench
// 3-5%, profiles/README.md); BRICKS=true tests m.bricks per lookup and
// serves both layouts.
template <bool BRICKS = true>
HD float grid_voxel(const MediumParams& m, const float* pool, int ix, int iy, int iz) {
    if constexpr (BRICKS) {
        if (m.bricks) {
            int b = m.bricks[(size_t(iz >> 3) * m.bny + (iy >> 3)) * m.bnx + (ix >> 3)];
            return b < 0 ? 0.f
                         : pool[size_t(b) * 512 + (((iz & 7) << 6) | ((iy & 7) << 3) | (ix & 7))];
        }
    }
    return pool[(size_t(iz) * m.ny + iy) * m.nx + ix];
}

template <bool BRICKS = true>
HD float grid_density_at(const MediumParams& m, const Vec3& p, Sampler* jitter) {
    Vec3 g = (p - m.grid_lo.xyz()) * m.grid_inv_extent.xyz();
    if (g.x < 0.f || g.y < 0.f || g.z < 0.f || g.x >= 1.f || g.y >= 1.f || g.z >= 1.f) return 0.f;
    float fx = g.x * m.nx, fy = g.y * m.ny, fz = g.z * m.nz;
    if (jitter) {
        // stochastic-offset nearest-neighbor (reference vol_grid.cu lookup):
        // unbiased trilinear in expectation at nearest-neighbor cost
        fx += jitter->next1f() - 0.5f;
        fy += jitter->next1f() - 0.5f;
        fz += jitter->next1f() - 0.5f;
    }
    int ix = clampv((int)fx, 0, m.nx - 1);
    int iy = clampv((int)fy, 0, m.ny - 1);
    int iz = clampv((int)fz, 0, m.nz - 1);
    return grid_voxel<BRICKS>(m, m.density, ix, iy, iz) * m.scale;
}

template <bool BRICKS = true>
HD float grid_temperature_at(const MediumParams& m, const Vec3& p) {
    if (!m.temperature) return 0.f;
    Vec3 g = (p - m.grid_lo.xyz()) * m.grid_inv_extent.xyz();
    if (g.x < 0.f || g.y < 0.f || g.z < 0.f || g.x >= 1.f || g.y >= 1.f || g.z >= 1.f) return 0.f;
    int ix = clampv((int)(g.x * m.nx), 0, m.nx - 1);
    int iy = clampv((int)(g.y * m.ny), 0, m.ny - 1);
    int iz = clampv((int)(g.z * m.nz), 0, m.nz - 1);
    return grid_voxel<BRICKS>(m, m.temperature, ix, iy, iz);
}

// ------------------------------------------------------- homogeneous medium
// Distance sampling with per-channel MIS and stable 3-channel weighting
// (reference homogeneous.cuh:43-83).
HD MediumSample homogeneous_sample(const MediumParams& m, float t_max, Sampler& sp) {
    MediumSample r{};
    Vec3 sig_s = m.sigma_s.xyz();
    Vec3 sig_t = m.sigma_a.xyz() + sig_s;
    if (sig_t.max_elem() <= 0.f) { r.local_thp = Vec3(1.f); r.scattered = false; return r; }
    // pick a channel uniformly
    int c = (int)(sp.next1f() * 3.f); c = c > 2 ? 2 : c;
    float st_c = fmaxf(c == 0 ? sig_t.x : (c == 1 ? sig_t.y : sig_t.z), 1e-8f);
    float t = -logf(fmaxf(1.f - sp.next1f(), 1e-12f)) / st_c;
    if (t < t_max) {
        Vec3 tr = (sig_t * -t).expv();
        Vec3 pdf_v = sig_t * tr;
        float pdf = (pdf_v.x + pdf_v.y + pdf_v.z) * (1.f / 3.f);
        r.local_thp = sig_s * tr / fmaxf(pdf, 1e-20f);
        r.dist = t;
        r.scattered = true;
    } else {
        Vec3 tr = (sig_t * -t_max).expv();
        float pdf = (tr.x + tr.y + tr.z) * (1.f / 3.f);
        r.local_thp = tr / fmaxf(pdf, 1e-20f);
        r.scattered = false;
    }
    return r;
}

HD Vec3 homogeneous_transmittance(const MediumParams& m, float dist) {
    Vec3 sig_t = m.sigma_a.xyz() + m.sigma_s.xyz();
    return (sig_t * -dist).expv();
}

// ------------------------------------------------------- majorant supergrid
// Amanatides-Woo DDA over the supercell grid: next() yields the ray
// segments [s0, s1) with their LOCAL majorants.  Delta/ratio tracking
// restart their exponential stepping at each boundary (memoryless), so
// per-segment majorants are unbiased and empty cells cost one DDA step.
struct SuperDDA {
    int cx, cy, cz, sx, sy, sz;
    int stx, sty, stz;
    float tmx, tmy, tmz;       // t of next boundary crossing per axis
    float tdx, tdy, tdz;       // t per cell step per axis
    float t_cur, t_end;
    const float* super;
    float scale;

    HD bool init(const MediumParams& m, const Ray& ray, float t_lim) {
        if (!m.super) return false;
        super = m.super; scale = m.scale;
        sx = m.sx; sy = m.sy; sz = m.sz;
        Vec3 lo = m.grid_lo.xyz();
        Vec3 inv_ext = m.grid_inv_extent.xyz();
        Vec3 inv_d = safe_rcp_dir(ray.d);
        float t0 = 0.f, t1 = t_lim;
        Vec3 cw;  // world size of one supercell per axis
        for (int a = 0; a < 3; ++a) {
            float ext = 1.f / inv_ext[a];
            float ta = (lo[a] - ray.o[a]) * inv_d[a];
            float tb = (lo[a] + ext - ray.o[a]) * inv_d[a];
            if (ta > tb) { float tt = ta; ta = tb; tb = tt; }
            t0 = fmaxf(t0, ta);
            t1 = fminf(t1, tb);
            cw.set(a, ext / (a == 0 ? (float)sx : a == 1 ? (float)sy : (float)sz));
        }
        t_cur = t0; t_end = t1;
        if (t0 >= t1) { t_end = t_cur; return true; }  // no overlap: empty march
        Vec3 p0 = ray.at(t0 + fminf(1e-5f, 0.5f * (t1 - t0)));
        int c[3];
        float tm[3], td[3];
        int st[3];
        for (int a = 0; a < 3; ++a) {
            int n = a == 0 ? sx : a == 1 ? sy : sz;
            float g = (p0[a] - lo[a]) / cw[a];
            c[a] = clampv((int)g, 0, n - 1);
            if (ray.d[a] > 0.f) {
                st[a] = 1;
                tm[a] = (lo[a] + (c[a] + 1) * cw[a] - ray.o[a]) * inv_d[a];
                td[a] = cw[a] * inv_d[a];
            } else if (ray.d[a] < 0.f) {
                st[a] = -1;
                tm[a] = (lo[a] + c[a] * cw[a] - ray.o[a]) * inv_d[a];
                td[a] = -cw[a] * inv_d[a];
            } else {
                st[a] = 0;
                tm[a] = MAX_DIST;
                td[a] = MAX_DIST;
            }
        }
        cx = c[0]; cy = c[1]; cz = c[2];
        stx = st[0]; sty = st[1]; stz = st[2];
        tmx = tm[0]; tmy = tm[1]; tmz = tm[2];
        tdx = td[0]; tdy = td[1]; tdz = td[2];
        return true;
    }

    HD bool next(float& s0, float& s1, float& maj) {
        if (t_cur >= t_end) return false;
        if (cx < 0 || cx >= sx || cy < 0 || cy >= sy || cz < 0 || cz >= sz) return false;
        maj = super[(size_t(cz) * sy + cy) * sx + cx] * scale;
        s0 = t_cur;
        float tn = fminf(fminf(tmx, tmy), tmz);
        s1 = fminf(tn, t_end);
        t_cur = s1;
        if (tn <= t_end) {
            if (tmx <= tmy && tmx <= tmz) { cx += stx; tmx += tdx; }
            else if (tmy <= tmz)          { cy += sty; tmy += tdy; }
            else                          { cz += stz; tmz += tdz; }
        }
        return true;
    }
};

// ------------------------------------------------------------- grid medium
// Delta-tracking distance sampling (reference vol_grid.cu:128-150), DDA'd
// over the majorant supergrid when present.
template <bool BRICKS = true>
HD MediumSample grid_sample(const MediumParams& m, const Ray& ray, float t_max, Sampler& sp) {
    MediumSample r{};
    r.local_thp = Vec3(1.f);
    float maj = m.majorant;
    if (maj <= 0.f) { r.scattered = false; return r; }
    float inv_maj = 1.f / maj;
    // colored single-scattering albedo: Russian roulette on the mean, tint
    // by albedo/mean on scatter (gray media: tint == 1, identical streams)
    Vec3 alb = m.sigma_s.xyz() /
               (m.sigma_s.xyz() + m.sigma_a.xyz()).maxv(Vec3(1e-8f));
    float a_mean = clampv((alb.x + alb.y + alb.z) * (1.f / 3.f), 1e-6f, 1.f);
    SuperDDA dda;
    if (dda.init(m, ray, t_max)) {
        float s0, s1, maj_c;
        int it = 0;
        while (dda.next(s0, s1, maj_c)) {
            if (maj_c <= 0.f) continue;               // empty supercell: free skip
            float inv_c = 1.f / maj_c;
            float t = s0;
            for (; it < 16384; ++it) {
                t -= logf(fmaxf(1.f - sp.next1f(), 1e-12f)) * inv_c;
                if (t >= s1) break;
                float dens = grid_density_at<BRICKS>(m, ray.at(t), &sp);
                if (sp.next1f() < dens * inv_c) {
                    if (sp.next1f() < a_mean) {
                        r.local_thp = alb * (1.f / a_mean);
                        r.dist = t;
                        r.scattered = true;
                        return r;
                    }
                    r.local_thp = Vec3(0.f);          // absorbed
                    return r;
                }
            }
        }
        r.scattered = false;
        return r;
    }
    float t = 0.f;
    for (int it = 0; it < 4096; ++it) {
        t -= logf(fmaxf(1.f - sp.next1f(), 1e-12f)) * inv_maj;
        if (t >= t_max) break;
        float dens = grid_density_at<BRICKS>(m, ray.at(t), &sp);
        float sig_t = dens;  // density IS sigma_t (scale folded in)
        if (sp.next1f() < sig_t * inv_maj) {
            // real collision: scatter with albedo, absorb otherwise
            if (sp.next1f() < a_mean) {
                r.local_thp = alb * (1.f / a_mean);
                r.dist = t;
                r.scattered = true;
                return r;
            }
            r.local_thp = Vec3(0.f);  // absorbed
            return r;
        }
        // null collision: continue
    }
    r.scattered = false;
    return r;
}

// Ratio-tracking transmittance with Russian roulette below Tr=0.1
// (reference vol_grid.cu:177-198); residual-ratio around avg_density when
// the control is useful (vol_grid.cu:153-175).
template <bool BRICKS = true>
HD Vec3 grid_transmittance(const MediumParams& m, const Ray& ray, float dist, Sampler& sp) {
    float maj = m.majorant;
    if (maj <= 0.f) return Vec3(1.f);
    SuperDDA dda;
    if (dda.init(m, ray, dist)) {
        float tr = 1.f;
        float s0, s1, maj_c;
        int it = 0;
        while (dda.next(s0, s1, maj_c)) {
            if (maj_c <= 0.f) continue;
            float inv_c = 1.f / maj_c;
            float t = s0;
            for (; it < 16384; ++it) {
                t -= logf(fmaxf(1.f - sp.next1f(), 1e-12f)) * inv_c;
                if (t >= s1) break;
                float dens = grid_density_at<BRICKS>(m, ray.at(t), &sp);
                tr *= fmaxf(0.f, 1.f - dens * inv_c);
                if (tr < 0.1f) {  // Russian roulette termination
                    if (sp.next1f() >= tr * 10.f) return Vec3(0.f);
                    tr = 0.1f;
                }
                if (tr <= 0.f) return Vec3(0.f);
            }
        }
        return Vec3(tr);
    }
    float inv_maj = 1.f / maj;
    float tr = 1.f;
    float t = 0.f;
    for (int it = 0; it < 4096; ++it) {
        t -= logf(fmaxf(1.f - sp.next1f(), 1e-12f)) * inv_maj;
        if (t >= dist) break;
        float dens = grid_density_at<BRICKS>(m, ray.at(t), &sp);
        tr *= fmaxf(0.f, 1.f - dens * inv_maj);
        if (tr < 0.1f) {  // Russian roulette termination
            if (sp.next1f() >= tr * 10.f) return Vec3(0.f);
            tr = 0.1f;
        }
        if (tr <= 0.f) return Vec3(0.f);
    }
    return Vec3(tr);
}

// ------------------------------------------------------------ dispatch API
template <bool BRICKS = true>
HD MediumSample medium_sample(const MediumParams& m, const Ray& ray, float t_max, Sampler& sp) {
    if (m.type == MED_HOMOGENEOUS) return homogeneous_sample(m, t_max, sp);
    return grid_sample<BRICKS>(m, ray, t_max, sp);
}

template <bool BRICKS = true>
HD Vec3 medium_transmittance(const MediumParams& m, const Ray& ray, float dist, Sampler& sp) {
    if (m.type == MED_HOMOGENEOUS) return homogeneous_transmittance(m, dist);
    return grid_transmittance<BRICKS>(m, ray, dist, sp);
}

// Blackbody emission at a point (temperature grid -> RGB, vol_grid.cu:97-102).
template <bool BRICKS = true>
HD Vec3 medium_emission(const MediumParams& m, const Vec3& p, Sampler& sp) {
    if (m.type != MED_GRID || !m.temperature || m.emission_scale <= 0.f) return Vec3(0.f);
    float T = grid_temperature_at<BRICKS>(m, p) * m.temp_scale;
    if (T < 100.f) return Vec3(0.f);
    return blackbody_rgb(T) * m.emission_scale;
}

} // namespace hippt
