"""Host variants of the traversal probe (tests/probe_util.py): the walks
behind scene_intersect / scene_occluded on host_sv against a numpy float64
brute force.  They prove the reference and its ambiguity filter before a GPU
is involved; tests/test_gpu_probe.py runs the same body on the device walks
(LDS/scratch split stack, LDS top-tree cache, fast-math).

Filtered rays per case (cap 3 %), as printed by the test:
a_single 0.10 %, b_random400 0.15 %, c_clustered3000 0.59 %,
c_clustered3000_sbvh 0.59 %, d_tris_spheres 0.05 %, e_slab1500 1.22 %.
"""
import numpy as np
import pytest

import probe_util as pu


@pytest.mark.parametrize("name", list(pu.CASES))
def test_host_walks_match_float64_brute_force(name):
    pu.check_walks(name, device=-1)


def test_reference_against_property_brute_force():
    """The reference agrees with tests/test_property.py's brute_force_t on
    the rays it does not call ambiguous (triangles, unbounded tmax)."""
    from test_property import brute_force_t
    rng = np.random.default_rng(3)
    tris = pu._tris_random(rng, 60)
    lo, hi = tris.reshape(-1, 3).min(axis=0), tris.reshape(-1, 3).max(axis=0)
    o, d = pu.make_rays(rng, lo.astype(np.float64), hi.astype(np.float64), 1e4)
    o, d = o[:300], d[:300]
    ref = pu.reference(tris, None, o, d, np.full(len(o), pu.MAX_DIST))
    n = 0
    for i in np.flatnonzero(~ref["ambiguous"]):
        t = brute_force_t(tris.astype(np.float64), o[i].astype(np.float64),
                          d[i].astype(np.float64))
        assert np.isfinite(t) == ref["hit"][i], i
        if ref["hit"][i]:
            assert abs(t - ref["t"][i]) <= 1e-9 * max(1.0, t), i
            n += 1
    assert n > 20


def test_filter_flags_edge_and_range_cases():
    """Rays built to sit on an edge, at EPSILON and at tmax are filtered;
    a ray through the middle is not."""
    tris = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], np.float32)
    d = np.array([[0, 0, -1.0]] * 5)
    o = np.array([[0.25, 0.25, 1.0],      # middle: clean hit at t=1
                  [0.5, 0.00005, 1.0],    # v within 1e-4 of 0
                  [0.25, 0.25, 0.0015],   # t within 1e-3 of EPSILON
                  [0.25, 0.25, 1.0],      # t within 1e-3*t of tmax
                  [0.25, 0.25, 1.0]])     # tmax well short: clean miss
    tmax = np.array([10.0, 10.0, 10.0, 1.0005, 0.5])
    ref = pu.reference(tris, None, o, d, tmax)
    assert ref["ambiguous"].tolist() == [False, True, True, True, False]
    assert ref["hit"][0] and ref["prim"][0] == 0 and abs(ref["t"][0] - 1.0) < 1e-12
    assert not ref["hit"][4]
