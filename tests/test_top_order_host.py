"""Host checks of the top-first node order of the traversal mirrors
(csrc/core/bvh4.h bvh4_top_first, through C.bvh4_top_first) and of the LDS
budget of the node cache at its built stride, on the trees of
tests/probe_util.py.

The order moves node indices only: boxes, leaf words, counts and slots are
the source node's, internal child words are the permuted source indices.

The exact invariant of the ordered part.  With K = min(n, n_top), position 0
is the root, and for k = 1 .. K-1 the node at position k is, among the open
nodes at that moment (internal children of the nodes at positions < k that
are not themselves at a position < k), the one with the highest priority,
the lower source index on a tie.  The priority of a node is
  level: minus its depth,
  area:  the surface area 2 (dx dy + dy dz + dz dx) of its box in its
         parent's slot, in float64 from the stored float32 bounds.
The area is recomputed here; the compiler may associate the three products
otherwise than numpy does, so a chosen node's area may fall short of the
largest open one by a relative 1e-12 (a few float64 ulps), no more.  Depths
are integers and compared exactly, ties included.
"""
import numpy as np
import pytest

from hippt import C
import probe_util as pu
import test_visit_host as tv  # noqa: F401  (registers the f_tris5 / g_tris16 cases)

TREES = tv.TREES
ORDERS = ["area", "level", "dfs"]
AREA_RTOL = 1e-12


def nodes4_of(name):
    return np.ascontiguousarray(pu.get_case(name)["scene"]._np["nodes4"], np.float32)


def n_tops(n):
    return sorted({0, 1, 2, 3, 5, max(n - 1, 0), n, n + 7})


def children(raw_i32):
    """(m,4) int64 child words of a BVH4 array viewed as int32."""
    return raw_i32[:, 24:28].astype(np.int64)


def slot_areas(nodes4):
    """(m,4) float64 surface area of every slot's box."""
    b = np.asarray(nodes4, np.float32)[:, :24].astype(np.float64).reshape(-1, 6, 4)
    dx, dy, dz = b[:, 3] - b[:, 0], b[:, 4] - b[:, 1], b[:, 5] - b[:, 2]
    a = 2.0 * (dx * dy + dy * dz + dz * dx)
    return np.where(a >= 0.0, a, 0.0)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", TREES)
def test_reordered_tree(name, order):
    src = nodes4_of(name)
    n = len(src)
    src_i = src.view(np.int32)
    src_ch = children(src_i)
    area = slot_areas(src)
    for n_top in n_tops(n):
        out, perm = C.bvh4_top_first(src, n_top, order)
        out = np.ascontiguousarray(out, np.float32)
        where = (name, order, n_top)
        assert out.shape == src.shape and perm.shape == (n,), where
        # a permutation that keeps the root
        assert sorted(perm.tolist()) == list(range(n)) and perm[0] == 0, where
        inv = np.empty(n, np.int64)
        inv[perm] = np.arange(n)                      # inv[new] = source
        out_i = out.view(np.int32)
        # boxes and counts bit for bit, in the same slots
        np.testing.assert_array_equal(out_i[:, :24], src_i[inv, :24], str(where))
        np.testing.assert_array_equal(out_i[:, 28:32], src_i[inv, 28:32], str(where))
        # leaf words untouched, internal words = permuted source child
        sch, och = src_ch[inv], children(out_i)
        leaf = sch < 0
        np.testing.assert_array_equal(och[leaf], sch[leaf], str(where))
        np.testing.assert_array_equal(och[~leaf], perm[sch[~leaf]], str(where))
        if order == "dfs" or n_top <= 1:
            np.testing.assert_array_equal(perm, np.arange(n), str(where))
            np.testing.assert_array_equal(out_i, src_i, str(where))
            continue
        K = min(n, n_top)
        # parent and depth of every source node
        parent = np.full(n, -1, np.int64)
        slot_of = np.full(n, -1, np.int64)
        for i in range(n):
            for c in range(4):
                if src_ch[i, c] >= 0:
                    parent[src_ch[i, c]] = i
                    slot_of[src_ch[i, c]] = c
        assert (parent[1:] >= 0).all() and parent[0] == -1, where
        depth = np.zeros(n, np.int64)
        for i in range(1, n):                          # pre-order: parent first
            assert parent[i] < i
            depth[i] = depth[parent[i]] + 1
        # every prefix of the ordered part is closed under "parent"
        for k in range(1, K):
            assert perm[parent[inv[k]]] < k, (where, k)
        # each position holds the best open node of its moment
        placed = np.zeros(n, bool)
        placed[0] = True
        for k in range(1, K):
            open_ = np.flatnonzero(~placed & placed[np.maximum(parent, 0)] & (parent >= 0))
            got = inv[k]
            assert got in open_, (where, k)
            if order == "level":
                best = min(open_, key=lambda i: (depth[i], i))
                assert got == best, (where, k)
            else:
                pr = area[parent[open_], slot_of[open_]]
                mine = area[parent[got], slot_of[got]]
                assert mine >= pr.max() * (1.0 - AREA_RTOL), (where, k)
                same = open_[pr == mine]
                assert got == same.min(), (where, k)
            placed[got] = True
        # the rest keeps its relative source order
        assert (np.diff(inv[K:]) > 0).all(), where


def test_argument_checks():
    src = nodes4_of("g_tris16")
    with pytest.raises(RuntimeError):
        C.bvh4_top_first(src, 4, "widest")
    with pytest.raises(RuntimeError):
        C.bvh4_top_first(src[:, :31], 4, "area")
    out, perm = C.bvh4_top_first(src)                  # defaults: the scene's order
    assert out.shape == src.shape and perm[0] == 0
    assert C.BVH4_TOP_ORDERED == 512


@pytest.mark.parametrize("name", ["b_random400", "e_slab1500"])
def test_area_order_moves_nodes(name):
    """The check above must not pass on an identity: on these trees the
    depth-first head is not the top, so both orders move nodes below 64."""
    src = nodes4_of(name)
    for order in ("area", "level"):
        _, perm = C.bvh4_top_first(src, 64, order)
        assert (perm[:64] != np.arange(64)).any(), (name, order)


_dfs_results = {}


def _trace(name, order, lds_n, monkeypatch):
    case = pu.get_case(name)
    if order is None:
        monkeypatch.delenv("HIPPT_TOP_ORDER", raising=False)
    else:
        monkeypatch.setenv("HIPPT_TOP_ORDER", order)
    scene = pu.build_scene(case["tris"], case["spheres"], False)
    return scene.trace_rays(case["o"], case["d"], case["tmax"], device=-1, lds_n=lds_n)


@pytest.mark.parametrize("order", ["area", "level", None])
@pytest.mark.parametrize("name", TREES)
def test_host_walks_same_under_every_order(name, order, monkeypatch):
    for lds_n in (0, 1, 3):
        key = (name, lds_n)
        if key not in _dfs_results:
            _dfs_results[key] = _trace(name, "dfs", lds_n, monkeypatch)
        got = _trace(name, order, lds_n, monkeypatch)
        for a, b in zip(got, _dfs_results[key]):
            np.testing.assert_array_equal(a, b, f"{name} {order} lds_n={lds_n}")


def test_unknown_order_is_an_error(monkeypatch):
    case = pu.get_case("a_single")
    monkeypatch.setenv("HIPPT_TOP_ORDER", "widest")
    with pytest.raises(RuntimeError):
        pu.build_scene(case["tris"], None, False)


@pytest.mark.parametrize("occ", [3, 4, 5, 6])
def test_plan_at_the_launchers_stride(occ):
    """The launchers pass C.TRAV_CACHE_STRIDE as node_bytes (128, or 144 in a
    HIPPT_CACHE_STRIDE=144 build): the cache plus four stack entries fit the
    occupancy's budget at every request."""
    stride = C.TRAV_CACHE_STRIDE
    assert stride >= 128 and stride % 16 == 0
    budget = {3: 26, 4: 20, 5: 16, 6: 12}[occ] * 2048
    for req in (0, 1, 16, 21, 32, 64, 128, 256, 512, 4096):
        lds_n, n_cached, shmem = C.lds_plan(occ, True, False, 100000, stride, req)
        assert n_cached == min(req, (budget - 4 * 2048) // stride)
        assert lds_n >= 4
        assert n_cached * stride + 4 * 2048 <= budget
        assert shmem == lds_n * 2048 + n_cached * stride <= budget
        # the cache never reaches past the top-first part of the array
        assert n_cached <= C.BVH4_TOP_ORDERED
