"""Shared pieces of the shade-table, shade-probe and shade-render tests:
small scenes that together reach every branch of the shading loaders
(csrc/core/shade_load.h, emitter.h LightPrim), and numpy recomputations of
the per-primitive shade word and the NEE light records from a scene's `_np`
arrays."""
import numpy as np

from hippt.scene.scene import (BsdfDesc, CameraDesc, EmitterDesc, ObjectDesc,
                               RenderConfig, Scene, SceneDesc)

SPHERE_BIT = np.uint32(0x80000000)
OBJ_MASK = np.uint32(0x000FFFFF)


# ---------------------------------------------------------------- references
def np_prim_shade(prim_obj, objs):
    """bit 31 sphere, bits 16-30 emitter_id + 1 (0 = none), bits 0-15 bsdf_id."""
    prim_obj = np.asarray(prim_obj, np.uint32)
    objs = np.asarray(objs, np.int32).reshape(-1, 8)
    oi = (prim_obj & OBJ_MASK).astype(np.int64)
    bsdf = objs[oi, 2].astype(np.uint32)
    em = (objs[oi, 3].astype(np.int64) + 1).clip(0).astype(np.uint32)
    return (prim_obj & SPHERE_BIT) | (em << np.uint32(16)) | bsdf


def np_light_prims(prims, attrs, prim_obj, emitter_prims):
    """(n, 32) uint32: 12 Prim words, 16 PrimAttr words, the sphere flag, 3 zero."""
    ep = np.asarray(emitter_prims, np.int64).reshape(-1)
    out = np.zeros((len(ep), 32), np.uint32)
    out[:, 0:12] = np.ascontiguousarray(prims, np.float32).view(np.uint32)[ep]
    out[:, 12:28] = np.ascontiguousarray(attrs, np.float32).view(np.uint32)[ep]
    out[:, 28] = np.asarray(prim_obj, np.uint32)[ep] & SPHERE_BIT
    return out


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


# -------------------------------------------------------------------- scenes
def _quad(p0, p1, p2, p3):
    return np.array([[p0, p1, p2], [p0, p2, p3]], np.float32)


def _room(rng, n=120):
    """Floor + a scattered triangle soup above it (several BVH leaves)."""
    floor = _quad((-4, 0, -4), (4, 0, -4), (4, 0, 4), (-4, 0, 4))
    soup = (rng.uniform(-2.5, 2.5, (n, 1, 3)) * np.array([1, 0.3, 1]) + np.array([0, 1.2, 0])
            + rng.normal(0, 0.25, (n, 3, 3))).astype(np.float32)
    return floor, soup


def _uvs(tris):
    """Planar uv from x,z so textured lookups vary over the mesh."""
    t = np.asarray(tris, np.float32).reshape(-1, 3, 3)
    return np.stack([t[..., 0] * 0.25 + 0.5, t[..., 2] * 0.25 + 0.5], axis=-1).astype(np.float32)


def _textures(rng):
    def tex(h, w, lo, hi):
        t = np.ones((h, w, 4), np.float32)
        t[..., :3] = rng.uniform(lo, hi, (h, w, 3))
        return t
    albedo = tex(8, 8, 0.2, 0.9)
    normal = tex(8, 8, 0.4, 0.6)
    normal[..., 2] = 1.0                      # mostly +z in tangent space
    rough = tex(4, 4, 0.15, 0.6)
    return [albedo, normal, rough]


def _camera(width, height):
    return CameraDesc(pos=(0.0, 2.2, -6.5), lookat=(0.0, 1.0, 0.0), fov=50.0,
                      width=width, height=height)


def spheres_scene(width=64, height=36, renderer="pt"):
    """Triangles and spheres; a sphere area emitter, a triangle area-spot
    emitter, a point light (so the selection CDF is present); a textured
    Lambertian, a GGX conductor with a normal map and a roughness texture,
    plastic, glass; two objects share one BSDF."""
    rng = np.random.default_rng(41)
    floor, soup = _room(rng)
    d = SceneDesc()
    d.textures = _textures(rng)
    d.bsdfs = [
        BsdfDesc(type="lambertian", kd=(0.7, 0.7, 0.7), textures={"diffuse": 0}),
        BsdfDesc(type="ggx", metal="Cu", roughness_x=0.3, roughness_y=0.2,
                 textures={"normal": 1, "roughness": 2}),
        BsdfDesc(type="plastic", kd=(0.8, 0.2, 0.2), ior=1.4, trans_scaler=0.9),
        BsdfDesc(type="translucent", ior=1.5),
        BsdfDesc(type="lambertian", kd=(0.9, 0.9, 0.9)),
    ]
    d.emitters = [
        EmitterDesc(type="area", emission=(1.0, 0.9, 0.8), scale=12.0),
        EmitterDesc(type="area-spot", emission=(0.8, 0.9, 1.0), scale=30.0, cos_max=0.7),
        EmitterDesc(type="point", emission=(1.0, 1.0, 1.0), scale=4.0, pos=(-2.5, 3.0, -2.0)),
    ]
    lamp = _quad((-0.6, 3.5, -0.6), (0.6, 3.5, -0.6), (0.6, 3.5, 0.6), (-0.6, 3.5, 0.6))
    balls = np.array([[-1.5, 0.5, -1.0, 0.5], [0.0, 0.5, -1.5, 0.5], [1.5, 0.5, -1.0, 0.5]],
                     np.float32)
    d.objects = [
        ObjectDesc(tris=floor, uvs=_uvs(floor), bsdf=0),
        ObjectDesc(tris=soup[:60], uvs=_uvs(soup[:60]), bsdf=1),
        ObjectDesc(tris=soup[60:], bsdf=2),
        ObjectDesc(spheres=balls[:1], bsdf=3),
        ObjectDesc(spheres=balls[1:], bsdf=2),                     # shares bsdf 2
        ObjectDesc(spheres=np.array([[2.2, 2.6, 0.5, 0.3], [-2.2, 2.4, 0.8, 0.25]], np.float32),
                   bsdf=4, emitter=0),                             # sphere emitter
        ObjectDesc(tris=lamp, bsdf=4, emitter=1),                  # area-spot, facing down
    ]
    d.camera = _camera(width, height)
    d.config = RenderConfig(renderer=renderer, max_depth=6, max_diffuse=4,
                            max_specular=6, max_transmit=6)
    return d


def no_emitter_scene():
    rng = np.random.default_rng(42)
    floor, soup = _room(rng, 40)
    d = SceneDesc()
    d.bsdfs = [BsdfDesc(type="lambertian"), BsdfDesc(type="specular")]
    d.objects = [ObjectDesc(tris=floor, bsdf=0), ObjectDesc(tris=soup, bsdf=1)]
    d.camera = _camera(16, 16)
    d.config = RenderConfig(renderer="pt")
    return d


def shared_bsdf_scene():
    """Two objects on one BSDF, one of them an emitter."""
    rng = np.random.default_rng(43)
    floor, soup = _room(rng, 30)
    d = SceneDesc()
    d.bsdfs = [BsdfDesc(type="lambertian", kd=(0.5, 0.6, 0.7))]
    d.emitters = [EmitterDesc(type="area", scale=5.0)]
    d.objects = [ObjectDesc(tris=floor, bsdf=0), ObjectDesc(tris=soup, bsdf=0, emitter=0)]
    d.camera = _camera(16, 16)
    d.config = RenderConfig(renderer="pt")
    return d


_SCENES = {}


def get_scene(name):
    """A built Scene by name, once per process."""
    if name not in _SCENES:
        if name == "cornell":
            from hippt.scene.procedural import cornell_box
            desc = cornell_box(width=32, height=32)
        else:
            desc = {"spheres": spheres_scene, "no_emitter": no_emitter_scene,
                    "shared_bsdf": shared_bsdf_scene}[name]()
        _SCENES[name] = Scene(desc)
    return _SCENES[name]


# --------------------------------------------------------------------- probe
def probe_queries(scene, n_max=256):
    """Primitive indices for shade_probe: the first and the last primitive,
    every sphere and emitter primitive that fits, non-emitters, a repeated
    index, the rest random."""
    po = scene._np["prim_obj"]
    objs = scene._np["objs"]
    n = len(po)
    word = np_prim_shade(po, objs)
    sph = np.flatnonzero(word & SPHERE_BIT)
    em = np.flatnonzero((word >> np.uint32(16)) & np.uint32(0x7FFF))
    non = np.flatnonzero(((word >> np.uint32(16)) & np.uint32(0x7FFF)) == 0)
    rng = np.random.default_rng(7)
    q = [0, n - 1, 0, n - 1]
    q += sph[:32].tolist() + em[:32].tolist() + non[:32].tolist()
    q += rng.integers(0, n, max(0, n_max - len(q))).tolist()
    return np.asarray(q[:n_max], np.int32), dict(sph=sph, em=em, non=non)


def check_probe(scene, device):
    """shade_probe on `device` against the scene's own tables, exactly."""
    q, kinds = probe_queries(scene)
    attr, word, bsdf, em = scene.shade_probe(q, device=device)
    tabs = scene.native.tables()
    ref_word = np_prim_shade(scene._np["prim_obj"], scene._np["objs"])
    np.testing.assert_array_equal(word, ref_word[q])
    np.testing.assert_array_equal(attr, u32(scene._np["attrs"])[q])
    bsdf_tab = np.asarray(tabs["bsdfs"])
    np.testing.assert_array_equal(bsdf, bsdf_tab[(ref_word[q] & np.uint32(0xFFFF)).astype(np.int64)])
    em_tab = np.asarray(tabs["emitters"])
    em_id = ((ref_word[q] >> np.uint32(16)) & np.uint32(0x7FFF)).astype(np.int64) - 1
    ref_em = np.zeros((len(q), 16), np.uint32)
    if len(em_tab):
        ref_em[em_id >= 0] = em_tab[em_id[em_id >= 0]]
    np.testing.assert_array_equal(em, ref_em)
    return q, kinds, (attr, word, bsdf, em)
