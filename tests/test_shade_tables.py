"""The two host-built shading tables against a numpy recomputation from the
scene's own arrays, bit for bit: the per-primitive shade word
(C.build_prim_shade) and the NEE light records (C.build_light_prims), both
the free builders and what finalize() put into the scene."""
import numpy as np
import pytest

from hippt import C
import shade_util as su


def _check_tables(name):
    scene = su.get_scene(name)
    a = scene._np
    ref_word = su.np_prim_shade(a["prim_obj"], a["objs"])
    ref_lp = su.np_light_prims(a["prims"], a["attrs"], a["prim_obj"], a["emitter_prims"])
    word = np.asarray(C.build_prim_shade(a["prim_obj"], a["objs"]))
    lp = np.asarray(C.build_light_prims(a["prims"], a["attrs"], a["prim_obj"],
                                        a["emitter_prims"]))
    assert word.dtype == np.uint32 and lp.dtype == np.uint32
    assert lp.shape == (len(a["emitter_prims"]), 32)
    np.testing.assert_array_equal(word, ref_word)
    np.testing.assert_array_equal(lp, ref_lp)
    tabs = scene.native.tables()
    np.testing.assert_array_equal(np.asarray(tabs["prim_shade"]), ref_word)
    np.testing.assert_array_equal(np.asarray(tabs["light_prims"]).reshape(-1, 32), ref_lp)
    return scene, ref_word, ref_lp


def test_cornell_triangle_emitter_in_bvh_order():
    scene, word, lp = _check_tables("cornell")
    order = scene._np["order"]
    assert (order != np.arange(len(order))).any(), "BVH order is the identity"
    em = (word >> np.uint32(16)) & np.uint32(0x7FFF)
    assert (em > 0).any() and (em == 0).any()
    assert len(lp) == int((em > 0).sum())
    assert not (word & su.SPHERE_BIT).any()
    # the emitter primitives are not a contiguous run starting at 0
    assert (scene._np["emitter_prims"] != np.arange(len(lp))).any()


def test_spheres_and_sphere_emitter():
    scene, word, lp = _check_tables("spheres")
    sph = (word & su.SPHERE_BIT) != 0
    em = (word >> np.uint32(16)) & np.uint32(0x7FFF)
    assert sph.sum() == 5
    assert (sph & (em == 1)).sum() == 2          # the sphere emitter, emitter 0
    assert (~sph & (em == 2)).sum() == 2         # the area-spot quad, emitter 1
    assert (lp[:, 28] == su.SPHERE_BIT).sum() == 2 and (lp[:, 28] == 0).sum() == 2
    assert (lp[:, 29:] == 0).all()


def test_no_emitter_gives_zero_records():
    scene, word, lp = _check_tables("no_emitter")
    assert lp.shape == (0, 32)
    assert ((word >> np.uint32(16)) == 0).all()
    assert set(np.unique(word & np.uint32(0xFFFF))) == {0, 1}


def test_two_objects_share_one_bsdf():
    scene, word, lp = _check_tables("shared_bsdf")
    assert ((word & np.uint32(0xFFFF)) == 0).all()
    em = (word >> np.uint32(16)) & np.uint32(0x7FFF)
    assert (em == 1).sum() == 30 and (em == 0).sum() == 2


def _objs(bsdf_id, emitter_id):
    o = np.zeros((1, 8), np.int32)
    o[0, 2], o[0, 3] = bsdf_id, emitter_id
    return o


def test_range_limits():
    po = np.zeros(3, np.uint32)
    w = np.asarray(C.build_prim_shade(po, _objs(65535, 32766)))
    assert (w == np.uint32(65535 | (32767 << 16))).all()
    with pytest.raises(RuntimeError):
        C.build_prim_shade(po, _objs(65536, -1))
    with pytest.raises(RuntimeError):
        C.build_prim_shade(po, _objs(0, 32767))


def test_tables_follow_objects_and_emitter_prims_set_after_finalize():
    """finalize() rebuilds both tables whenever objects or emitter
    primitives were set since the last build, and only then fails on an id
    that does not fit."""
    from hippt.scene.scene import Scene
    scene = Scene(su.shared_bsdf_scene())        # own scene: it is modified
    a, nat = scene._np, scene.native
    before = np.asarray(nat.tables()["prim_shade"]).copy()
    # objects: the emitter object loses its emitter, the floor gets bsdf 7
    objs = a["objs"].copy()
    objs[0, 2], objs[1, 3] = 7, -1
    nat.set_objects(objs)
    word = np.asarray(nat.tables()["prim_shade"])
    np.testing.assert_array_equal(word, su.np_prim_shade(a["prim_obj"], objs))
    assert (word != before).any()
    # emitter primitives: a shorter, reversed list
    ep = a["emitter_prims"][::-1][:5].copy()
    nat.set_emitter_prims(ep, np.linspace(0.2, 1.0, 5).astype(np.float32))
    lp = np.asarray(nat.tables()["light_prims"]).reshape(-1, 32)
    np.testing.assert_array_equal(lp, su.np_light_prims(a["prims"], a["attrs"],
                                                        a["prim_obj"], ep))
    # geometry: prim_obj reversed -> both tables follow
    po = np.ascontiguousarray(a["prim_obj"][::-1])
    pr, at = np.ascontiguousarray(a["prims"][::-1]), np.ascontiguousarray(a["attrs"][::-1])
    nat.set_geometry(pr, at, po, a["nodes"], a["nodes4"], np.zeros((0, 64), np.float32))
    tabs = nat.tables()
    np.testing.assert_array_equal(np.asarray(tabs["prim_shade"]), su.np_prim_shade(po, objs))
    np.testing.assert_array_equal(np.asarray(tabs["light_prims"]).reshape(-1, 32),
                                  su.np_light_prims(pr, at, po, ep))
    # an id that does not fit is refused at the next finalize
    bad = objs.copy()
    bad[0, 2] = 65536
    nat.set_objects(bad)
    with pytest.raises(RuntimeError):
        nat.finalize()
