"""Host checks of the straight-line any-hit visit (csrc/core/bvh4.h:
BVH_VISIT_ANY4, compiled into the walk when BVH4_ANY_STRAIGHT is set) and of
the leaf loops that read the whole primitive first, on the trees and rays of
tests/probe_util.py.

* visit equivalence: C.bvh4_any_visit_selftest runs, for every (ray, node)
  pair, one visit child by child (the form the walk runs) and one in a
  straight line, each on an empty private stack, and compares {next} and the
  pushed words as sets: the same words, none twice, no BVH4_NONE_W pushed.
  The order is deliberately not compared: the any-hit walk returns a
  predicate that no visiting order can change;
* split stack: the any-hit walk with the bottom 0..3 stack entries in the
  strided stand-in for LDS, so the three unrolled pushes cross the boundary
  at every position, on a tree where nearly every child is hit and on one
  with spheres (the sphere path of the leaf loops);
* last leaf: a ray reaches the leaf that ends the primitive array, which is
  where a leaf loop that reads ahead must not read past the end.
"""
import numpy as np
import pytest

from hippt import C
import probe_util as pu


def _tris_few(rng, n):
    # few large triangles: vertices anywhere in the 10^3 box
    return rng.uniform(-5, 5, (n, 3, 3)).astype(np.float32)


# the 5- and 16-triangle trees of tests/test_visit_host.py, registered the
# same way (whichever module is imported first defines them)
pu.CASES.setdefault("f_tris5", (159, lambda r: (_tris_few(r, 5), None), False, 1e4))
pu.CASES.setdefault("g_tris16", (32, lambda r: (_tris_few(r, 16), None), False, 1e4))

NONE_W = 0x7FFFFFFF
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
    """Rays starting inside every filled child box of the root, so that all
    of them are hit; None if those boxes do not meet."""
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


def test_tree_shapes():
    """What the small trees are there for: three empty slots in the single
    triangle's root, an internal child next to empty slots in the 5-triangle
    tree."""
    w1 = child_words(pu.get_case("a_single")["scene"]._np["nodes4"])
    assert len(w1) == 1 and (w1[0] == NONE_W).sum() == 3
    w5 = child_words(pu.get_case("f_tris5")["scene"]._np["nodes4"])
    assert ((w5[0] < 0x80000000) & (w5[0] != NONE_W)).sum() == 1
    assert (w5 == NONE_W).any()


@pytest.mark.parametrize("name", TREES)
def test_any_visit_equivalence(name):
    case = pu.get_case(name)
    nodes4 = case["scene"]._np["nodes4"]
    o, d = case["o"], case["d"]
    extra = root_overlap_rays(nodes4, np.random.default_rng(77))
    if extra is not None:
        o, d = np.concatenate([o, extra[0]]), np.concatenate([d, extra[1]])
    for tmax in TMAX:
        assert C.bvh4_any_visit_selftest(nodes4, o, d, tmax) == 0, (name, tmax)


def test_any_visit_equivalence_all_four_hit():
    """Origins inside all four child boxes of the root: four hit words, all
    three pushes.  The boxes of a built root need not meet in one place, so
    the root of the 16-triangle tree gets four different boxes around one
    cube (the construction of tests/test_visit_host.py)."""
    rng = np.random.default_rng(78)
    nodes4 = np.array(pu.get_case("g_tris16")["scene"]._np["nodes4"], np.float32)
    assert (child_words(nodes4)[0] != NONE_W).all()
    nodes4[0, 0:12] = -1.0 - rng.uniform(0.5, 3.0, 12)
    nodes4[0, 12:24] = 1.0 + rng.uniform(0.5, 3.0, 12)
    o, d = root_overlap_rays(nodes4, rng, n=256)
    assert ((o > nodes4[0, 0:12].reshape(3, 4).max(axis=1)) &
            (o < nodes4[0, 12:24].reshape(3, 4).min(axis=1))).all()
    for tmax in TMAX:
        assert C.bvh4_any_visit_selftest(nodes4, o, d, tmax) == 0


def test_any_visit_zero_prim_leaf():
    """A leaf of no prims that keeps its box is hit like any child and must
    be dropped by its word, not pushed."""
    case = pu.get_case("g_tris16")
    nodes4 = np.array(case["scene"]._np["nodes4"], np.float32)
    raw = nodes4.view(np.int32)
    raw[0, 24 + 1] = ~5
    raw[0, 28 + 1] = 0
    assert child_words(nodes4)[0, 1] == NONE_W
    for tmax in TMAX:
        assert C.bvh4_any_visit_selftest(nodes4, case["o"], case["d"], tmax) == 0


@pytest.mark.parametrize("lds_n", [0, 1, 2, 3])
@pytest.mark.parametrize("name", ["e_slab1500", "d_tris_spheres"])
def test_any_hit_split_stack(name, lds_n):
    pu.check_walks(name, device=-1, lds_n=lds_n)
    case = pu.get_case(name)
    sc = case["scene"]
    assert sc.last_trace_plan == (lds_n, 0)
    occ = sc.trace_rays(case["o"], case["d"], case["tmax"], device=-1, lds_n=lds_n)[4]
    ref = sc.trace_rays(case["o"], case["d"], case["tmax"], device=-1, lds_n=0)[4]
    np.testing.assert_array_equal(occ, ref)


@pytest.mark.parametrize("name", ["a_single", "f_tris5"])
def test_last_leaf_of_prim_array_is_reached(name):
    case = pu.get_case(name)
    sc = case["scene"]
    n_prims = len(sc._np["prims"])
    raw = np.ascontiguousarray(sc._np["nodes4"], np.float32).view(np.int32)
    child, cnt = raw[:, 24:28].ravel(), raw[:, 28:32].ravel()
    leaf = (child < 0) & (cnt > 0)
    base, end = ~child[leaf], ~child[leaf] + cnt[leaf]
    assert end.max() == n_prims
    last = int(base[end.argmax()])          # the leaf with base + cnt == n_prims
    t, prim, u, v, occ = sc.trace_rays(case["o"], case["d"], case["tmax"], device=-1)
    in_last = (prim >= last) & (prim < n_prims)
    print(f"{name}: {n_prims} prims, last leaf [{last}, {n_prims}), "
          f"{int(in_last.sum())} rays hit it")
    assert in_last.sum() > 0
    assert occ[in_last].all()               # the any-hit walk got there too
