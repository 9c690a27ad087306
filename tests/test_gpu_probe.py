"""Device probes: the wavefront counting sort against numpy, and the device
BVH4 walks (LDS/scratch split stack, LDS top-tree cache, tri_only, fast-math)
against the float64 brute force of tests/probe_util.py — the same body that
tests/test_probe_host.py runs on the host walks."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU visible", allow_module_level=True)

from hippt import C  # noqa: E402
import probe_util as pu  # noqa: E402

DEAD = 0x80
NONE = np.uint32(0xFFFFFFFF)
WHOLE = 1 << 20   # n_cached request larger than any tree here


# ------------------------------------------------------------ counting sort
def sort_reference(status, gather, mode):
    ent = status if gather is None else status[gather & np.uint32(0x00FFFFFF)]
    top = ent >> np.uint32(24)
    key = np.where(top >= DEAD, DEAD, 0) if mode else top
    live = key < DEAD
    return ent[live], int(live.sum())


def check_sort(status, gather, mode):
    status = np.ascontiguousarray(status, np.uint32)
    g = np.zeros(0, np.uint32) if gather is None else np.ascontiguousarray(gather, np.uint32)
    ref_live, n_live = sort_reference(status, gather, mode)
    out, live = C.wf_sort_probe(status, g, mode)
    out = np.asarray(out)
    assert live == n_live, (live, n_live)
    np.testing.assert_array_equal(np.sort(out[:live]), np.sort(ref_live))
    if mode == 0:
        keys = out[:live] >> np.uint32(24)
        assert (np.diff(keys.astype(np.int64)) >= 0).all()
    assert (out[live:] == NONE).all(), "written beyond the live prefix"
    out2, live2 = C.wf_sort_probe(status, g, mode)   # cursors re-zeroed
    assert live2 == live
    np.testing.assert_array_equal(np.sort(np.asarray(out2)[:live2]), np.sort(ref_live))


def make_status(kind, n, rng):
    payload = rng.permutation(n).astype(np.uint32)
    if kind == "all_dead":
        top = rng.choice(np.array([0x80, 0x81, 0xC3, 0xFF], np.uint32), n)
    elif kind == "one_key":
        top = np.full(n, 37, np.uint32)
    elif kind == "uniform":
        top = rng.integers(0, 64, n).astype(np.uint32)
        top[rng.random(n) < 0.3] = DEAD
    elif kind == "edge_bytes":
        top = rng.choice(np.array([0x00, 0x7F, 0x80, 0x81, 0xFF], np.uint32), n)
    else:
        raise ValueError(kind)
    return (top << np.uint32(24)) | payload


SORT_SIZES = [1, 255, 256, 257, 4095, 4096, 4097, 3 * 4096 + 7]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n", SORT_SIZES)
def test_counting_sort_matches_numpy(n, mode):
    rng = np.random.default_rng(1000 + n)
    for kind in ["all_dead", "one_key", "uniform", "edge_bytes"]:
        check_sort(make_status(kind, n, rng), None, mode)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n", SORT_SIZES)
def test_counting_sort_gather_matches_numpy(n, mode):
    """Second and later sorts: the pass runs over a previous order view whose
    entries carry stale top bytes (masked off) and re-reads the fresh status
    byte, which says dead for a third of them."""
    rng = np.random.default_rng(2000 + n)
    for kind in ["uniform", "edge_bytes"]:
        # status in pixel order, as the trace kernels write it
        top = make_status(kind, n, rng) >> np.uint32(24)
        status = (top << np.uint32(24)) | np.arange(n, dtype=np.uint32)
        for m in sorted({1, min(300, n), n}):
            idx = rng.choice(n, m, replace=False).astype(np.uint32)
            redead = idx[rng.random(m) < 1.0 / 3.0]
            st = status.copy()
            st[redead] = (np.uint32(DEAD) << np.uint32(24)) | redead
            stale = rng.integers(0, 256, m).astype(np.uint32) << np.uint32(24)
            check_sort(st, stale | idx, mode)


# ------------------------------------------------------------ device walks
# (case, lds_n, n_cached); -1 = the render launcher's own value
WALK_PARAMS = [
    ("a_single", 0, 0), ("a_single", -1, -1), ("a_single", 1, 1),
    ("b_random400", 0, 0), ("b_random400", 1, 1), ("b_random400", 2, WHOLE),
    ("b_random400", -1, -1), ("b_random400", 1, -1), ("b_random400", -1, 0),
    ("c_clustered3000", 1, -1), ("c_clustered3000", -1, -1), ("c_clustered3000", 0, 0),
    ("c_clustered3000_sbvh", 1, -1), ("c_clustered3000_sbvh", -1, -1),
    ("d_tris_spheres", 0, -1), ("d_tris_spheres", 1, 0), ("d_tris_spheres", 2, 1),
    ("d_tris_spheres", -1, -1),
    ("e_slab1500", 1, -1), ("e_slab1500", -1, -1), ("e_slab1500", 2, 0),
    ("e_slab1500", 0, 0),
]


@pytest.mark.parametrize("name,lds_n,n_cached", WALK_PARAMS)
def test_device_walks_match_float64_brute_force(name, lds_n, n_cached):
    pu.check_walks(name, device=0, lds_n=lds_n, n_cached=n_cached)
    scene = pu.get_case(name)["scene"]
    used_lds, used_cache = scene.last_trace_plan
    n_nodes4 = scene.bvh_stats["n_nodes4"]
    if lds_n >= 0:
        assert used_lds == lds_n
    else:
        assert used_lds >= 4          # the launcher always leaves 4 entries
    if n_cached == WHOLE:
        assert used_cache == n_nodes4  # the whole tree sits in LDS
    elif n_cached >= 0:
        assert used_cache == min(n_cached, n_nodes4)
    else:
        assert 0 < used_cache <= n_nodes4
