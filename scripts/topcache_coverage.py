#!/usr/bin/env python
"""Share of BVH4 node visits an LDS node cache of a given size would serve.

CPU only.  Builds a scene, orders its BVH4 the way the traversal mirrors are
ordered (C.bvh4_top_first) and runs a Python copy of the ordered pop-culling
closest-hit walk (csrc/core/bvh4.h bvh_closest_ww) over sample rays: camera
rays, then for each further generation rays from the previous generation's
hit points in uniformly random directions.  For every prefix size it prints,
per generation, the share of all node visits whose node index lies below the
prefix, i.e. in the cache.  The walk visits the same boxes in the same order
under every node order, so one walk serves all orders: only the indices the
visits are counted under differ.

    python scripts/topcache_coverage.py kitchen
    python scripts/topcache_coverage.py sports-car --orders area --prefixes 32 64
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

EPSILON = 1e-3
MAX_DIST = 1e7
SPHERE_BIT = 0x80000000


def camera_rays(cam, n, rng):
    pos = np.asarray(cam.pos, np.float64)
    fwd = np.asarray(cam.lookat, np.float64) - pos
    fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, np.asarray(cam.up, np.float64))
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    tan = np.tan(np.radians(cam.fov) * 0.5)
    sx = rng.uniform(-1, 1, n) * tan
    sy = rng.uniform(-1, 1, n) * tan * cam.height / cam.width
    d = fwd[None] + sx[:, None] * right[None] + sy[:, None] * up[None]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.repeat(pos[None], n, axis=0), d


def leaf_hit(prims, prim_obj, base, cnt, o, d, t_best):
    p = prims[base:base + cnt].astype(np.float64)
    v0, e1, e2 = p[:, 0:3], p[:, 4:7], p[:, 8:11]
    sph = (prim_obj[base:base + cnt] & SPHERE_BIT) != 0
    pv = np.cross(d[None], e2)
    det = (e1 * pv).sum(axis=1)
    ok = np.abs(det) > 1e-12
    inv = 1.0 / np.where(ok, det, 1.0)
    tv = o[None] - v0
    u = (tv * pv).sum(axis=1) * inv
    qv = np.cross(tv, e1)
    v = (qv * d[None]).sum(axis=1) * inv
    t = (e2 * qv).sum(axis=1) * inv
    hit = ok & ~sph & (u >= 0) & (v >= 0) & (u + v <= 1)
    if sph.any():
        oc = o[None] - v0
        b = (oc * d[None]).sum(axis=1)
        disc = b * b - ((oc * oc).sum(axis=1) - p[:, 3] ** 2)
        s = np.sqrt(np.maximum(disc, 0.0))
        ts = np.where(-b - s > EPSILON, -b - s, -b + s)
        t = np.where(sph, ts, t)
        hit = np.where(sph, disc >= 0, hit)
    t = np.where(hit & (t > EPSILON) & (t < t_best), t, np.inf)
    return float(t.min()) if len(t) else np.inf


def walk(nodes, child, cnt, prims, prim_obj, o, d, visits):
    """Ordered walk with leaves postponed onto the stack and entries culled
    on pop against the closest hit so far; appends visited node indices."""
    with np.errstate(divide="ignore"):
        inv_d = 1.0 / np.where(d == 0.0, 1e-30, d)
    t_best = MAX_DIST
    stack = [(0.0, 0, 0)]                       # (t_near, is_leaf, word)
    while stack:
        t_near, is_leaf, w = stack.pop()
        if t_near >= t_best:
            continue
        if is_leaf:
            base, pc = w
            t_best = min(t_best, leaf_hit(prims, prim_obj, base, pc, o, d, t_best))
            continue
        visits.append(w)
        box = nodes[w]
        t0 = (box[0:3] - o[:, None]) * inv_d[:, None]
        t1 = (box[3:6] - o[:, None]) * inv_d[:, None]
        enter = np.maximum(np.minimum(t0, t1).max(axis=0), 0.0)
        exit_ = np.minimum(np.maximum(t0, t1).min(axis=0), t_best)
        hit = [c for c in range(4) if enter[c] <= exit_[c]
               and not (child[w, c] < 0 and cnt[w, c] == 0)]
        for c in sorted(hit, key=lambda c: (enter[c], c), reverse=True):   # far first
            ch = int(child[w, c])
            if ch < 0:
                stack.append((float(enter[c]), 1, (~ch, int(cnt[w, c]))))
            else:
                stack.append((float(enter[c]), 0, ch))
    return t_best


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("scene", nargs="?", default="kitchen",
                    choices=["kitchen", "sports-car", "cornell"])
    ap.add_argument("--orders", nargs="+", default=["dfs", "level", "area"])
    ap.add_argument("--prefixes", nargs="+", type=int, default=[16, 32, 64, 128, 256])
    ap.add_argument("--rays", type=int, default=400, help="rays per generation")
    ap.add_argument("--generations", type=int, default=4)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()

    import hippt
    from hippt.scene import procedural
    from hippt.scene.scene import Scene

    gens = {"kitchen": procedural.kitchen, "sports-car": procedural.sports_car,
            "cornell": procedural.cornell_box}
    desc = gens[args.scene](renderer="pt")
    scene = Scene(desc)
    nodes4 = np.ascontiguousarray(scene._np["nodes4"], np.float32)
    raw = nodes4.view(np.int32)
    child, cnt = raw[:, 24:28].astype(np.int64), raw[:, 28:32].astype(np.int64)
    # (m, 6, 4): lo xyz, hi xyz of every slot
    boxes = nodes4[:, :24].astype(np.float64).reshape(-1, 6, 4)
    prims = np.asarray(scene._np["prims"], np.float32)
    prim_obj = np.asarray(scene._np["prim_obj"], np.uint32)

    rng = np.random.default_rng(args.seed)
    o, d = camera_rays(desc.camera, args.rays, rng)
    per_gen = []                                # visited source indices per generation
    for g in range(args.generations):
        visits, hits = [], []
        n_rays = len(o)
        for i in range(n_rays):
            t = walk(boxes, child, cnt, prims, prim_obj, o[i], d[i], visits)
            if t < MAX_DIST:
                hits.append(o[i] + t * d[i])
        per_gen.append((np.asarray(visits, np.int64), n_rays))
        if not hits:
            break
        src = np.asarray(hits)[rng.integers(0, len(hits), args.rays)]
        nd = rng.normal(size=(args.rays, 3))
        d = nd / np.linalg.norm(nd, axis=1, keepdims=True)
        o = src + 1e-3 * d

    n = len(nodes4)
    print(f"{args.scene}: {n} BVH4 nodes, {len(prims)} prims, "
          f"{args.rays} rays x {len(per_gen)} generations, visits/ray "
          + " ".join(f"{len(v) / max(r, 1):.1f}" for v, r in per_gen))
    print("| prefix | " + " | ".join(args.orders) + " |")
    print("|---|" + "---|" * len(args.orders))
    perms = {}
    for order in args.orders:
        _, perm = hippt.C.bvh4_top_first(nodes4, hippt.C.BVH4_TOP_ORDERED, order)
        perms[order] = np.asarray(perm, np.int64)
    for k in args.prefixes:
        cells = []
        for order in args.orders:
            shares = [100.0 * (perms[order][v] < k).mean() for v, _ in per_gen if len(v)]
            cells.append(f"{min(shares):.0f}-{max(shares):.0f} %")
        print(f"| {k} | " + " | ".join(cells) + " |")


if __name__ == "__main__":
    main()
