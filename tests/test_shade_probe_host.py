"""Scene.shade_probe on the host: the records the shading loaders
(csrc/core/shade_load.h) gather for a hit, against the scene's tables,
exactly.  tests/test_gpu_shade_probe.py runs the same body on the device."""
import numpy as np
import pytest

import shade_util as su


@pytest.mark.parametrize("name", ["cornell", "spheres", "no_emitter", "shared_bsdf"])
def test_host_probe_matches_tables(name):
    scene = su.get_scene(name)
    q, kinds, (attr, word, bsdf, em) = su.check_probe(scene, device=-1)
    assert len(q) <= 256 and q[0] == 0 and q[1] == len(scene._np["prim_obj"]) - 1
    assert q[2] == q[0]                                   # a repeated index
    np.testing.assert_array_equal(attr[2], attr[0])
    is_em = np.isin(q, kinds["em"])
    assert (em[~is_em] == 0).all()
    if name == "spheres":
        assert np.isin(q, kinds["sph"]).any() and is_em.any() and (~is_em).any()
        assert (em[is_em] != 0).any(axis=1).all()
        # anchor the BSDF words to the description: type at word 12, kd first
        desc = scene.desc
        ids = (word & np.uint32(0xFFFF)).astype(int)
        k = int(np.flatnonzero(ids == 2)[0])
        assert bsdf[k, 12] == 3                            # plastic
        np.testing.assert_array_equal(bsdf[k, 0:3].view(np.float32),
                                      np.asarray(desc.bsdfs[2].kd, np.float32))
        k = int(np.flatnonzero(ids == 1)[0])
        tex = bsdf[k, 16:20].view(np.int16)
        assert tex[3] == 1 and tex[4] == 2 and tex[0] == -1   # normal, roughness slots


def test_emitter_and_bsdf_words_match_the_description():
    """The probe's BSDF and emitter words against the scene description and
    the scene's numpy arrays, not against the holder's own tables."""
    scene = su.get_scene("spheres")
    desc, a = scene.desc, scene._np
    q, kinds, (attr, word, bsdf, em) = su.check_probe(scene, device=-1)
    ids = (word & np.uint32(0xFFFF)).astype(int)
    em_id = ((word >> np.uint32(16)) & np.uint32(0x7FFF)).astype(int) - 1
    # expected per-emitter prim_base / prim_cnt / inv_area from the arrays
    ref_word = su.np_prim_shade(a["prim_obj"], a["objs"])
    ref_em = ((ref_word >> np.uint32(16)) & np.uint32(0x7FFF)).astype(int) - 1
    types = {"point": 1, "area": 2, "area-spot": 3, "envmap": 4}
    base = 0
    expect = {}
    for e, ed in enumerate(desc.emitters):
        cnt = int((ref_em == e).sum())
        expect[e] = (base, cnt)
        base += cnt
    assert base == len(a["emitter_prims"])
    seen = set()
    for k in range(len(q)):
        b = desc.bsdfs[ids[k]]
        assert bsdf[k, 12] == {"lambertian": 0, "ggx": 5, "plastic": 3, "translucent": 2}[b.type]
        if b.type in ("lambertian", "plastic"):
            np.testing.assert_array_equal(bsdf[k, 0:3].view(np.float32),
                                          np.asarray(b.kd, np.float32))
        e = em_id[k]
        if e < 0:
            continue
        seen.add(e)
        ed = desc.emitters[e]
        np.testing.assert_array_equal(em[k, 0:3].view(np.float32),
                                      np.asarray(ed.emission, np.float32))
        assert em[k, 3:4].view(np.float32)[0] == np.float32(ed.scale)
        assert em[k, 8] == types[ed.type]
        assert int(em[k, 9].view(np.int32)) == int(np.flatnonzero(
            [o.emitter == e for o in desc.objects])[0])             # obj_id
        assert int(em[k, 10].view(np.int32)) == -1                   # no emission texture
        assert (int(em[k, 11]), int(em[k, 12])) == expect[e]          # prim_base, prim_cnt
        prims_e = a["emitter_prims"][expect[e][0]:expect[e][0] + expect[e][1]]
        assert (ref_em[prims_e] == e).all()
        # inv_area against the primitives' own areas
        pr = a["prims"][prims_e]
        sph = (a["prim_obj"][prims_e] & su.SPHERE_BIT) != 0
        area = np.where(sph, 4 * np.pi * pr[:, 3].astype(np.float64) ** 2,
                        0.5 * np.linalg.norm(np.cross(pr[:, 4:7], pr[:, 8:11]), axis=1))
        np.testing.assert_allclose(em[k, 13:14].view(np.float32)[0], 1.0 / area.sum(), rtol=1e-5)
        if ed.type == "area-spot":
            assert em[k, 7:8].view(np.float32)[0] == np.float32(ed.cos_max)
    assert seen == {0, 1}          # the sphere emitter and the area-spot quad


def test_probe_rejects_bad_index():
    scene = su.get_scene("cornell")
    n = len(scene._np["prim_obj"])
    with pytest.raises(RuntimeError):
        scene.shade_probe([n], device=-1)
    with pytest.raises(RuntimeError):
        scene.shade_probe([-1], device=-1)
