"""Shared body of the traversal probe tests (tests/test_probe_host.py runs it
on the host walks, tests/test_gpu_probe.py on the device walks): scenes, ray
sets, a numpy float64 brute-force reference with an ambiguity filter, and the
comparison of Scene.trace_rays against it.

Reference.  Every ray is tested against every primitive in float64 (Möller-
Trumbore for triangles as in tests/test_property.py, the quadratic roots for
spheres); a candidate counts when EPSILON < t < tmax.

Ambiguity filter.  A ray is left out when float32 could legitimately decide
otherwise.  Each candidate is classed twice: SURE (inside the primitive and
the t range with a margin) and MAYBE (inside when the margins are given
away).  The reference answer is the closest SURE candidate.  A ray is
ambiguous when a MAYBE-but-not-SURE candidate lies in front of that answer
(it could change hit/miss, t, the primitive or the any-hit verdict), or when
some triangle has |det| < 1e-7.  The margins are
  * barycentrics: u, v, 1-u-v within UV_TOL = 1e-4 of 0.  For a far origin
    the float32 rounding of (o - v0) alone is larger than that, so the margin
    is max(1e-4, 2^-21 |o-v0| |d x e2| / |det|): 2^-21 is 8 float32 ulps, the
    product is the size of the terms that cancel in u = (o-v0).(d x e2)/det.
    Within a few units of the geometry this stays at 1e-4; 1e4 away it grows
    to ~5e-3/|e1|, which is what float32 really resolves from there;
  * t: within 1e-3*max(1,t) of EPSILON or of tmax;
  * spheres: the float32 discriminant b^2 - (|oc|^2 - r^2) cancels, so it is
    uncertain by 2^-21 (b^2 + |oc|^2); a root is SURE only when the
    discriminant clears that and the resulting error of t stays inside half
    the t tolerance.
The primitive id alone is additionally not compared when a second candidate
lies within 1e-3*max(1,t) behind the closest one.
At most MAX_FILTERED = 3 % of the rays of a case may be left out.

Far rays and spheres.  From 1e4 away the float32 sphere discriminant is
uncertain by ~16 against r^2 <= 0.3: intersect_sphere cannot resolve a
sphere from there at all, and every such ray would be filtered (3.1 % of the
rays by themselves).  In the sphere scene (d) the far rays therefore start
1e2 away; the triangle-only scenes keep 1e4.
"""
import numpy as np

from hippt.scene.scene import (BsdfDesc, CameraDesc, ObjectDesc, RenderConfig,
                               Scene, SceneDesc)

EPSILON = 1e-3          # csrc/core/hd.h
MAX_DIST = 1e7
UV_TOL = 1e-4
DET_TOL = 1e-7
T_REL = 1e-3            # the bound of tests/test_property.py
MAX_FILTERED = 0.03
N_RAYS = 2048
F32_8ULP = 2.0 ** -21


# ------------------------------------------------------------------ scenes
def _tris_single(rng):
    return np.array([[[-1.0, -0.7, 0.2], [1.3, -0.4, -0.3], [0.1, 1.1, 0.4]]], np.float32)


def _tris_random(rng, n=400):
    # as test_bvh4_vs_bruteforce / test_property: scattered soup
    return (rng.uniform(-5, 5, (n, 1, 3)) + rng.normal(0, 0.7, (n, 3, 3))).astype(np.float32)


def _tris_clustered(rng, n=3000):
    centers = rng.uniform(-4, 4, (n // 16, 3))
    base = centers[rng.integers(0, len(centers), n)]
    return (base[:, None, :] + rng.normal(0, 0.25, (n, 3, 3))).astype(np.float32)


def _tris_slab(rng, n=1500):
    # every triangle reaches from below z=-1 to above z=+1 and spans a good
    # part of the 10x10 footprint: all boxes overlap in the slab |z|<1, so
    # nearly every child of every node is hit and the stack runs deep
    v = rng.uniform(-5, 5, (n, 3, 3))
    v[:, 0, 2] = rng.uniform(-3, -1, n)
    v[:, 1, 2] = rng.uniform(1, 3, n)
    v[:, 2, 2] = rng.uniform(-3, 3, n)
    return v.astype(np.float32)


def _spheres(rng, n=100):
    s = np.empty((n, 4), np.float32)
    s[:, :3] = rng.uniform(-5, 5, (n, 3))
    s[:, 3] = rng.uniform(0.15, 0.55, n)
    return s


# name -> (seed, builder(rng) -> (tris, spheres or None), use_sbvh, far distance)
CASES = {
    "a_single": (11, lambda r: (_tris_single(r), None), False, 1e4),
    "b_random400": (12, lambda r: (_tris_random(r), None), False, 1e4),
    "c_clustered3000": (13, lambda r: (_tris_clustered(r), None), False, 1e4),
    "c_clustered3000_sbvh": (13, lambda r: (_tris_clustered(r), None), True, 1e4),
    "d_tris_spheres": (14, lambda r: (_tris_random(r, 300), _spheres(r)), False, 1e2),
    "e_slab1500": (15, lambda r: (_tris_slab(r), None), False, 1e4),
}


def build_scene(tris, spheres, use_sbvh):
    d = SceneDesc()
    d.bsdfs = [BsdfDesc(type="lambertian")]
    d.objects = [ObjectDesc(tris=tris, bsdf=0)]
    if spheres is not None:
        d.objects.append(ObjectDesc(spheres=spheres, bsdf=0))
    d.camera = CameraDesc(pos=(0, 0, -20), lookat=(0, 0, 0), width=8, height=8)
    d.config = RenderConfig(renderer="pt", use_sbvh=use_sbvh)
    return Scene(d)


# -------------------------------------------------------------------- rays
def make_rays(rng, lo, hi, far):
    """(o, d) float32, N_RAYS of them: random origins aimed at random points
    of the scene box, plus 64 each of axis-aligned (signed zeros in the zero
    components), origin inside the box, origin `far` away, and missing the
    box altogether."""
    lo = lo - 0.05
    hi = hi + 0.05
    c, ext = 0.5 * (lo + hi), 0.5 * (hi - lo)
    n = N_RAYS

    def unit(v):
        return v / np.linalg.norm(v, axis=1, keepdims=True)

    target = rng.uniform(lo, hi, (n, 3))
    o = c + rng.uniform(-1, 1, (n, 3)) * (1.6 * ext + 1.0)
    d = unit(target - o)
    # axis-aligned, +0.0 / -0.0 in the zero components
    k = np.arange(64)
    axis = k % 3
    sign = np.where((k // 3) % 2 == 0, 1.0, -1.0)
    zero = np.where((k // 6) % 2 == 0, 0.0, -0.0)
    da = np.repeat(zero[:, None], 3, axis=1)
    da[k, axis] = sign
    oa = target[:64].copy()
    oa[k, axis] = c[axis] - sign * (ext[axis] * 1.5 + 1.0)
    o[0:64], d[0:64] = oa, da
    # origin inside the scene box
    o[64:128] = rng.uniform(lo, hi, (64, 3))
    d[64:128] = unit(rng.normal(size=(64, 3)))
    # far away, aimed at the box
    df = unit(rng.normal(size=(64, 3)))
    o[128:192], d[128:192] = target[128:192] - far * df, df
    # miss the box: start beyond the +++ corner, head further out
    o[192:256] = hi + rng.uniform(0.5, 3.0, (64, 3))
    d[192:256] = unit(np.abs(rng.normal(size=(64, 3))) + 0.05)
    o32, d32 = o.astype(np.float32), d.astype(np.float32)
    d32[0:64] = da.astype(np.float32)   # exact axes, keep the signed zeros
    return o32, d32


# --------------------------------------------------------------- reference
def _t_tol(t):
    return T_REL * np.maximum(1.0, np.abs(t))


def reference(tris, spheres, o, d, tmax, chunk=256):
    """float64 brute force.  tris (T,3,3), spheres (S,4) or None, o/d (R,3),
    tmax (R,).  Returns dict of per-ray arrays: hit, t, prim (index into
    tris then spheres), occluded, ambiguous, prim_ambiguous."""
    tris = np.asarray(tris, np.float64)
    o = np.asarray(o, np.float64)
    d = np.asarray(d, np.float64)
    tmax = np.asarray(tmax, np.float64)
    R, T = len(o), len(tris)
    v0, e1, e2 = tris[:, 0], tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
    out = dict(hit=np.zeros(R, bool), t=np.full(R, np.inf), prim=np.full(R, -1),
               ambiguous=np.zeros(R, bool), prim_ambiguous=np.zeros(R, bool))
    for r0 in range(0, R, chunk):
        sl = slice(r0, min(R, r0 + chunk))
        oo, dd, tm = o[sl, None, :], d[sl, None, :], tmax[sl, None]
        pv = np.cross(dd, e2[None])
        det = np.einsum("tj,rtj->rt", e1, pv)
        small = np.abs(det) < DET_TOL
        inv = 1.0 / np.where(det == 0.0, 1.0, det)
        tv = oo - v0[None]
        u = np.einsum("rtj,rtj->rt", tv, pv) * inv
        qv = np.cross(tv, e1[None])
        v = np.einsum("rtj,rtj->rt", np.broadcast_to(dd, qv.shape), qv) * inv
        t = np.einsum("tj,rtj->rt", e2, qv) * inv
        bary = np.minimum(np.minimum(u, v), 1.0 - u - v)
        uv_tol = np.maximum(UV_TOL, F32_8ULP * np.linalg.norm(tv, axis=2)
                            * np.linalg.norm(pv, axis=2) * np.abs(inv))
        tt = _t_tol(t)
        sure = ~small & (bary > uv_tol) & (t > EPSILON + tt) & (t < tm - tt)
        maybe = ~small & (bary >= -uv_tol) & (t > EPSILON - tt) & (t < tm + tt)
        cand_t = [t]
        cand_sure = [sure]
        cand_maybe = [maybe]
        cand_prim = [np.broadcast_to(np.arange(T)[None], t.shape)]
        amb = small.any(axis=1)
        if spheres is not None:
            sp = np.asarray(spheres, np.float64)
            oc = oo - sp[None, :, :3]
            a = np.einsum("rsj,rsj->rs", np.broadcast_to(dd, oc.shape),
                          np.broadcast_to(dd, oc.shape))
            b = np.einsum("rsj,rsj->rs", oc, np.broadcast_to(dd, oc.shape))
            oc2 = np.einsum("rsj,rsj->rs", oc, oc)
            disc = b * b - a * (oc2 - sp[None, :, 3] ** 2)
            dtol = F32_8ULP * (b * b + oc2)
            s = np.sqrt(np.maximum(disc, 0.0))
            dt = dtol / np.maximum(2.0 * s, 1e-300)     # error of a root
            for root in ((-b - s) / a, (-b + s) / a):
                tt = _t_tol(root)
                sure_s = (disc > dtol) & (dt < 0.5 * tt) & \
                    (root > EPSILON + tt) & (root < tm - tt)
                slack = tt + np.sqrt(dtol)
                maybe_s = (disc > -dtol) & (root > EPSILON - slack) & (root < tm + slack)
                cand_t.append(root)
                cand_sure.append(sure_s)
                cand_maybe.append(maybe_s)
                cand_prim.append(np.broadcast_to(T + np.arange(len(sp))[None], root.shape))
        ct = np.concatenate(cand_t, axis=1)
        cs = np.concatenate(cand_sure, axis=1)
        cm = np.concatenate(cand_maybe, axis=1)
        cp = np.concatenate(cand_prim, axis=1)
        ts = np.where(cs, ct, np.inf)
        best = ts.argmin(axis=1)
        rows = np.arange(ts.shape[0])
        t_best = ts[rows, best]
        hit = np.isfinite(t_best)
        p_best = np.where(hit, cp[rows, best], -1)
        unsure = cm & ~cs
        amb |= (unsure & (ct < t_best[:, None])).any(axis=1)
        near = cm & (ct < (t_best + _t_tol(t_best))[:, None]) & (cp != p_best[:, None])
        out["hit"][sl] = hit
        out["t"][sl] = t_best
        out["prim"][sl] = p_best
        out["ambiguous"][sl] = amb
        out["prim_ambiguous"][sl] = near.any(axis=1) & hit
    out["occluded"] = out["hit"].copy()
    return out


# -------------------------------------------------------------------- cases
_CASE_CACHE = {}


def get_case(name):
    """Scene + rays + reference of a case, built once per process."""
    if name in _CASE_CACHE:
        return _CASE_CACHE[name]
    seed, builder, use_sbvh, far = CASES[name]
    rng = np.random.default_rng(seed)
    tris, spheres = builder(rng)
    scene = build_scene(tris, spheres, use_sbvh)
    pts = tris.reshape(-1, 3).astype(np.float64)
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    if spheres is not None:
        lo = np.minimum(lo, (spheres[:, :3] - spheres[:, 3:4]).min(axis=0))
        hi = np.maximum(hi, (spheres[:, :3] + spheres[:, 3:4]).max(axis=0))
    o, d = make_rays(rng, lo, hi, far)
    # tmax: a quarter of the rays stop at half the reference hit distance
    # (must miss), a quarter at 1.5x (must still hit), the rest unbounded
    free = reference(tris, spheres, o, d, np.full(len(o), MAX_DIST))
    tmax = np.full(len(o), MAX_DIST, np.float32)
    idx = np.arange(len(o))
    short = free["hit"] & (idx % 4 == 0)
    longer = free["hit"] & (idx % 4 == 1)
    tmax[short] = (0.5 * free["t"][short]).astype(np.float32)
    tmax[longer] = (1.5 * free["t"][longer]).astype(np.float32)
    ref = reference(tris, spheres, o, d, tmax)
    keep = ~ref["ambiguous"]
    # the reference itself: short rays miss, longer rays hit what they hit before
    assert not ref["hit"][short & keep & ~free["ambiguous"]].any()
    sel = longer & keep & ~free["ambiguous"]
    assert ref["hit"][sel].all() and (ref["prim"][sel] == free["prim"][sel]).all()
    case = dict(name=name, scene=scene, tris=tris, spheres=spheres, o=o, d=d, tmax=tmax,
                ref=ref, n_short=int(short.sum()), n_long=int(longer.sum()))
    _CASE_CACHE[name] = case
    return case


def check_walks(name, device, lds_n=-1, n_cached=-1):
    """Scene.trace_rays on `device` against the float64 reference of a case."""
    case = get_case(name)
    scene, ref = case["scene"], case["ref"]
    tris = np.asarray(case["tris"], np.float64)
    n_tris = len(tris)
    o, d, tmax = case["o"], case["d"], case["tmax"]
    t, prim, u, v, occ = scene.trace_rays(o, d, tmax, device=device, lds_n=lds_n,
                                          n_cached=n_cached)
    keep = ~ref["ambiguous"]
    filtered = 1.0 - keep.mean()
    print(f"{name} device={device} lds_n={lds_n} n_cached={n_cached}: "
          f"{100 * filtered:.2f}% of {len(o)} rays filtered, "
          f"{int(ref['hit'][keep].sum())} hits, {case['n_short']} short, "
          f"{case['n_long']} long, plan={getattr(scene, 'last_trace_plan', None)}")
    assert filtered <= MAX_FILTERED, f"{name}: {filtered:.4f} of the rays are ambiguous"
    assert ref["hit"][keep].sum() > 0.2 * keep.sum() or name == "a_single"
    assert ref["hit"][keep].sum() > 100

    got_hit = prim >= 0
    bad = keep & (got_hit != ref["hit"])
    assert not bad.any(), (name, "hit/miss differs", np.flatnonzero(bad)[:8],
                           t[bad][:8], ref["t"][bad][:8])
    bad = keep & (occ != ref["occluded"])
    assert not bad.any(), (name, "occluded differs", np.flatnonzero(bad)[:8])
    assert (t[keep & ~got_hit] > 1e6).all()       # a miss reports MAX_DIST

    h = keep & ref["hit"]
    tol = T_REL * np.maximum(1.0, ref["t"][h])
    err = np.abs(t[h].astype(np.float64) - ref["t"][h])
    assert (err <= tol).all(), (name, "t", float((err / tol).max()))
    # primitive id: map the BVH-ordered index back to the source primitive
    order = scene._np["order"]
    src = order[prim[h]]
    pid_ok = (src == ref["prim"][h]) | ref["prim_ambiguous"][h]
    assert pid_ok.all(), (name, "prim", np.flatnonzero(h)[~pid_ok][:8])
    # barycentrics place the hit where the reference ray does (triangles)
    tri = h.copy()
    tri[h] = (src < n_tris) & (src == ref["prim"][h])
    tv = tris[ref["prim"][tri]]
    uu, vv = u[tri].astype(np.float64)[:, None], v[tri].astype(np.float64)[:, None]
    p_dev = tv[:, 0] + uu * (tv[:, 1] - tv[:, 0]) + vv * (tv[:, 2] - tv[:, 0])
    p_ref = o[tri].astype(np.float64) + ref["t"][tri][:, None] * d[tri].astype(np.float64)
    perr = np.linalg.norm(p_dev - p_ref, axis=1)
    ptol = T_REL * np.maximum(1.0, ref["t"][tri])
    assert (perr <= ptol).all(), (name, "hit point", float((perr / ptol).max()))
    return filtered
