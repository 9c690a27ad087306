"""Host checks of the (key, word) pair form of the width-4 visit
(csrc/core/bvh4.h: BVH_PAIR4, BVH_PAIR_MINMAX, BVH_VISIT_TAGGED4) on
hand-built nodes: the places where carrying the word beside its key through
the sort could differ from finding it again from the slot bits.

C.bvh4_visit_selftest runs, per (ray, node) pair, the ordered visit on the
BVH4Node (run-time count, select by slot) and the pair form on the tagged
node and compares `next` and every pushed entry; C.bvh4_any_visit_selftest
does the same for the any-hit visits as sets.  Both return the number of
mismatching pairs.

The nodes are single (1,32) records: boxes SoA, child[4], cnt[4].  Children
are slabs across the z axis, so a ray along +z through their common xy
footprint enters child c at exactly lo_z[c] (o_z = 0, d_z = 1), and random
rays hit any subset of them.
"""
import numpy as np
import pytest

from hippt import C

MAX_DIST = 1e7
EMPTY = (-1, 0)          # child ~0, no prims: what collapse_bvh4 writes
FAR = 1e6                # a point box no ray of the tests reaches


def node(z, children, xy=2.0):
    """One BVH4Node row.  z: four (lo_z, hi_z) or None for a box far away;
    children: four (child, cnt)."""
    row = np.zeros((1, 32), np.float32)
    raw = row.view(np.int32)
    for c in range(4):
        if z[c] is None:
            lo, hi = (FAR, FAR, FAR), (FAR, FAR, FAR)
        else:
            lo, hi = (-xy, -xy, z[c][0]), (xy, xy, z[c][1])
        for a in range(3):
            row[0, 4 * a + c] = lo[a]
            row[0, 12 + 4 * a + c] = hi[a]
        raw[0, 24 + c], raw[0, 28 + c] = children[c]
    return row


def leaf(base, cnt):
    return (~base, cnt)


def rays_for(rng, n=300):
    """+z rays through the footprint from z = 0 (exact enter distances), the
    same from inside and behind the slabs, and random rays around them."""
    k = 24
    o_ax = np.zeros((k, 3))
    o_ax[:, :2] = rng.uniform(-1.5, 1.5, (k, 2))
    o_ax[:, 2] = np.repeat([0.0, 5.5, 20.0], k // 3)
    d_ax = np.tile([0.0, 0.0, 1.0], (k, 1))
    d_ax[k // 2:, 2] = -1.0
    o = rng.uniform(-6, 6, (n, 3))
    o[:, 2] = rng.uniform(-4, 16, n)
    target = np.column_stack([rng.uniform(-2.5, 2.5, (n, 2)), rng.uniform(0, 12, n)])
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (np.concatenate([o_ax, o]).astype(np.float32),
            np.concatenate([d_ax, d]).astype(np.float32))


FILLED = [(7, 0), leaf(40, 3), (9, 0), leaf(100, 15)]
BELOW5 = float(np.nextafter(np.float32(5.0), np.float32(0.0)))

# name -> (node row, tmax values)
NODES = {
    # slot 0 is empty, its box is hit first: next must be BVH4_NONE_W (a
    # pop), the three real children are pushed
    "empty_nearest": (node([(1, 2), (3, 4), (5, 6), (7, 8)],
                           [EMPTY, leaf(40, 3), (9, 0), leaf(100, 15)]), [MAX_DIST, 3.5]),
    # an empty slot between two hit children, and one as the farthest
    "empty_between": (node([(1, 2), (3, 4), (5, 6), (7, 8)],
                           [(7, 0), EMPTY, leaf(9, 2), EMPTY]), [MAX_DIST, 5.5]),
    # bit-equal enter: only the slot bits order the children
    "equal_enter_2": (node([(3, 4), (5, 9), (5, 7), (1, 2)], FILLED), [MAX_DIST, 6.0]),
    "equal_enter_3": (node([(5, 6), (5, 9), (1, 2), (5, 7)], FILLED), [MAX_DIST, 6.0]),
    "equal_enter_4": (node([(5, 6), (5, 9), (5, 8), (5, 7)], FILLED), [MAX_DIST, 6.0]),
    "equal_enter_4_one_empty": (node([(5, 6), (5, 9), (5, 8), (5, 7)],
                                     [(7, 0), EMPTY, (9, 0), leaf(3, 1)]), [MAX_DIST]),
    "all_missed": (node([None, None, None, None], FILLED), [MAX_DIST, 0.0]),
    "all_empty_all_hit": (node([(1, 2), (3, 4), (5, 6), (7, 8)], [EMPTY] * 4), [MAX_DIST]),
    # the +z rays from z = 0 enter child 2 at exactly 5: hit at tmax = 5,
    # missed one ulp below
    "tmax_edge": (node([(1, 2), (3, 4), (5, 6), (7, 8)], FILLED), [5.0, BELOW5]),
    # a leaf of no prims keeps its box and its child index: dropped by its word
    "zero_prim_leaf": (node([(3, 4), (1, 2), (5, 6), (7, 8)],
                            [(7, 0), leaf(5, 0), leaf(9, 2), (11, 0)]), [MAX_DIST, 3.5]),
    "zero_prim_leaf_only": (node([None, (1, 2), None, None],
                                 [(7, 0), leaf(5, 0), leaf(9, 2), (11, 0)]), [MAX_DIST]),
}


@pytest.fixture(scope="module")
def rays():
    return rays_for(np.random.default_rng(2024))


def test_axis_rays_enter_where_the_cases_say(rays):
    """The +z rays from z = 0 run inside every footprint, so `enter` of a
    slab [lo_z, hi_z] is exactly lo_z: what equal_enter_* and tmax_edge
    rely on."""
    o, d = rays
    ax = (o[:, 2] == 0) & (d[:, 2] == 1)
    assert ax.sum() >= 4 and (np.abs(o[ax, :2]) < 2).all()
    assert (d[ax, :2] == 0).all()
    assert np.float32(BELOW5) < np.float32(5.0)
    assert np.nextafter(np.float32(BELOW5), np.float32(9.0)) == np.float32(5.0)


@pytest.mark.parametrize("name", sorted(NODES))
def test_pair_visit_matches_ordered_visit(name, rays):
    nodes4, tmaxes = NODES[name]
    o, d = rays
    for tmax in tmaxes:
        assert C.bvh4_visit_selftest(nodes4, o, d, tmax) == 0, (name, tmax)


@pytest.mark.parametrize("name", sorted(NODES))
def test_any_visit_same_children(name, rays):
    nodes4, tmaxes = NODES[name]
    o, d = rays
    for tmax in tmaxes:
        assert C.bvh4_any_visit_selftest(nodes4, o, d, tmax) == 0, (name, tmax)


def test_all_nodes_in_one_array(rays):
    # the same records as one (m,32) array: every ray against every node
    nodes4 = np.concatenate([NODES[k][0] for k in sorted(NODES)])
    o, d = rays
    for tmax in (MAX_DIST, 6.0, 5.0, BELOW5, 1e-3, 0.0):
        assert C.bvh4_visit_selftest(nodes4, o, d, tmax) == 0, tmax
        assert C.bvh4_any_visit_selftest(nodes4, o, d, tmax) == 0, tmax
