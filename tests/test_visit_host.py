"""Host checks of the tagged traversal node and the branch-free width-4 visit
(csrc/core/bvh4.h: BVH4NodeT, BVH_VISIT_TAGGED4) against the BVH4Node forms
they replaced on the device, on the trees and rays of tests/probe_util.py.

* visit equivalence: C.bvh4_visit_selftest runs, for every (ray, node) pair,
  one visit the BVH4Node way (run-time key count, compare-and-swap network,
  push loop, per-child tagging) and one the tagged way, each on an empty
  private stack, and compares `next` and every pushed 64-bit entry exactly;
* tagging: every slot of C.bvh4_tag against bvh4_child_word computed here;
* split stack: the walks with the bottom 0..3 stack entries in the strided
  stand-in for LDS, so the unrolled pushes cross the boundary at every
  position.
"""
import numpy as np
import pytest

from hippt import C
import probe_util as pu

NONE_W = 0x7FFFFFFF


def _tris_few(rng, n):
    # few large triangles: vertices anywhere in the 10^3 box
    return rng.uniform(-5, 5, (n, 3, 3)).astype(np.float32)


# the 5- and 16-triangle trees.  Seed 159 is the first of 100..399 whose
# 5-triangle tree has the shape test_small_tree_shapes asks for and whose
# rays hit often enough for pu.check_walks (23 % of them; the float64
# reference leaves out 0.05 % as ambiguous)
pu.CASES.setdefault("f_tris5", (159, lambda r: (_tris_few(r, 5), None), False, 1e4))
pu.CASES.setdefault("g_tris16", (32, lambda r: (_tris_few(r, 16), None), False, 1e4))

TREES = ["a_single", "f_tris5", "g_tris16", "b_random400", "e_slab1500"]
TMAX = [0.0, pu.EPSILON, 3.0, pu.MAX_DIST]


def child_words(nodes4):
    """bvh4_child_word of every slot of a (m,32) BVH4 array, in numpy."""
    raw = np.ascontiguousarray(nodes4, np.float32).view(np.int32)
    child, cnt = raw[:, 24:28].astype(np.int64), raw[:, 28:32].astype(np.int64)
    leaf = (0x80000000 | (cnt << 27) | (~child & 0xFFFFFFFF)) & 0xFFFFFFFF
    w = np.where(child < 0, leaf, child)
    return np.where((child < 0) & (cnt == 0), NONE_W, w).astype(np.uint32)


def root_overlap_rays(nodes4, rng, n=64):
    """Rays starting inside every filled child box of the root (all t_near are
    0, only the slot orders the keys), or None if those boxes do not meet."""
    root = np.asarray(nodes4, np.float32)[0]
    filled = child_words(nodes4)[0] != NONE_W
    lo = root[0:12].reshape(3, 4)[:, filled].max(axis=1)
    hi = root[12:24].reshape(3, 4)[:, filled].min(axis=1)
    if not (lo < hi).all():
        return None
    o = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return o, d


def test_small_tree_shapes():
    """What the small cases are there for: the 5-triangle tree has a root
    with one internal child and a node with empty slots (a collapsed root
    that has an empty slot itself has leaves only), the single triangle a
    root with three empty slots."""
    w = child_words(pu.get_case("f_tris5")["scene"]._np["nodes4"])
    assert len(w) == 2
    assert ((w[0] < 0x80000000) & (w[0] != NONE_W)).sum() == 1
    assert (w == NONE_W).any()
    w1 = child_words(pu.get_case("a_single")["scene"]._np["nodes4"])
    assert len(w1) == 1 and (w1[0] == NONE_W).sum() == 3


@pytest.mark.parametrize("name", TREES)
def test_tagged_words_match_child_word(name):
    nodes4 = pu.get_case(name)["scene"]._np["nodes4"]
    t = np.asarray(C.bvh4_tag(nodes4))
    assert t.shape == (len(nodes4), 32) and t.dtype == np.uint32
    raw = np.ascontiguousarray(nodes4, np.float32).view(np.uint32)
    np.testing.assert_array_equal(t[:, :24], raw[:, :24])      # boxes, bit for bit
    np.testing.assert_array_equal(t[:, 24:28], child_words(nodes4))
    assert (t[:, 28:32] == 0).all()


def zero_prim_leaf_tree():
    """The 16-triangle tree with slot 1 of the root turned into a leaf of no
    prims that keeps its box: hit like any child, dropped by its word."""
    nodes4 = np.array(pu.get_case("g_tris16")["scene"]._np["nodes4"], np.float32)
    raw = nodes4.view(np.int32)
    raw[0, 24 + 1] = ~5
    raw[0, 28 + 1] = 0
    return nodes4


def test_tagged_words_zero_prim_leaf():
    nodes4 = zero_prim_leaf_tree()
    t = np.asarray(C.bvh4_tag(nodes4))
    assert t[0, 25] == NONE_W
    np.testing.assert_array_equal(t[:, 24:28], child_words(nodes4))


@pytest.mark.parametrize("name", TREES)
def test_visit_equivalence(name):
    case = pu.get_case(name)
    nodes4 = case["scene"]._np["nodes4"]
    o, d = case["o"], case["d"]
    extra = root_overlap_rays(nodes4, np.random.default_rng(77))
    if extra is not None:
        o, d = np.concatenate([o, extra[0]]), np.concatenate([d, extra[1]])
    for tmax in TMAX:
        assert C.bvh4_visit_selftest(nodes4, o, d, tmax) == 0, (name, tmax)


def test_visit_equivalence_slot_order_only():
    """Origins inside all four child boxes of the root: every t_near is 0
    and only the slot in the low key bits orders the children.  The boxes of
    a built root need not meet in one place (e_slab1500's do not), so the
    root of the 16-triangle tree gets four different boxes around one cube."""
    rng = np.random.default_rng(78)
    nodes4 = np.array(pu.get_case("g_tris16")["scene"]._np["nodes4"], np.float32)
    assert (child_words(nodes4)[0] != NONE_W).all()
    nodes4[0, 0:12] = -1.0 - rng.uniform(0.5, 3.0, 12)
    nodes4[0, 12:24] = 1.0 + rng.uniform(0.5, 3.0, 12)
    o, d = root_overlap_rays(nodes4, rng, n=256)
    assert ((o > nodes4[0, 0:12].reshape(3, 4).max(axis=1)) &
            (o < nodes4[0, 12:24].reshape(3, 4).min(axis=1))).all()
    for tmax in TMAX:
        assert C.bvh4_visit_selftest(nodes4, o, d, tmax) == 0


def test_visit_equivalence_zero_prim_leaf():
    nodes4 = zero_prim_leaf_tree()
    case = pu.get_case("g_tris16")
    for tmax in TMAX:
        assert C.bvh4_visit_selftest(nodes4, case["o"], case["d"], tmax) == 0


@pytest.mark.parametrize("lds_n", [0, 1, 2, 3])
@pytest.mark.parametrize("name", ["b_random400", "e_slab1500"])
def test_split_stack(name, lds_n):
    case = pu.get_case(name)
    sc = case["scene"]
    n = sc._np
    # (the scene's binary tree carries one sentinel row past its end)
    assert C.bvh4_selftest(n["prims"], n["prim_obj"], n["nodes"][:-1], n["nodes4"],
                           case["o"], case["d"], 1e7, lds_n=lds_n) == 0
    pu.check_walks(name, device=-1, lds_n=lds_n)
    assert sc.last_trace_plan == (lds_n, 0)
    got = sc.trace_rays(case["o"], case["d"], case["tmax"], device=-1, lds_n=lds_n)
    ref = sc.trace_rays(case["o"], case["d"], case["tmax"], device=-1, lds_n=0)
    for a, b in zip(got, ref):
        np.testing.assert_array_equal(a, b)
