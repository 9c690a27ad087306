"""Device side of tests/test_top_order_host.py: the walks read the first
n_cached nodes of a top-first traversal array from the LDS copy, and
neither the order, the cache size nor the stack split may change a result.

* Probe: Scene.trace_rays(device=0) on scenes built under every
  HIPPT_TOP_ORDER, at cache sizes around the root (0, 1, 2), below and at the
  level-order top (5, 21) and at the default (64), with one stack entry in
  LDS and with the launcher's own split: all five result arrays equal those
  of the depth-first build without a cache.
* Images: tests/occ_worker.py renders the small kitchen once per
  configuration, each in a process of its own (HIPPT_TOPCACHE is read once
  per process) under its own timeout; after the first worker that fails no
  further one is started.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU visible", allow_module_level=True)

import probe_util as pu  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "occ_worker.py")
SCENES = ["b_random400", "e_slab1500"]

_scenes = {}      # (case, order) -> uploaded Scene
_reference = {}   # case -> result arrays of the dfs build at k = 0, lds_n = 1


def scene_of(name, order):
    key = (name, order)
    if key not in _scenes:
        case = pu.get_case(name)
        old = os.environ.get("HIPPT_TOP_ORDER")
        os.environ["HIPPT_TOP_ORDER"] = order
        try:
            scene = pu.build_scene(case["tris"], case["spheres"], False)
        finally:
            if old is None:
                del os.environ["HIPPT_TOP_ORDER"]
            else:
                os.environ["HIPPT_TOP_ORDER"] = old
        scene.upload(0)
        _scenes[key] = scene
    return _scenes[key]


def trace(name, order, lds_n, k):
    case = pu.get_case(name)
    scene = scene_of(name, order)
    out = scene.trace_rays(case["o"], case["d"], case["tmax"], device=0, lds_n=lds_n,
                           n_cached=k)
    return out, scene.last_trace_plan


def reference_of(name):
    if name not in _reference:
        out, plan = trace(name, "dfs", 1, 0)
        assert plan == (1, 0)
        assert (out[1] >= 0).sum() > 100               # the rays do hit
        _reference[name] = out
    return _reference[name]


@pytest.mark.parametrize("order", ["area", "level", "dfs"])
@pytest.mark.parametrize("name", SCENES)
def test_walks_same_at_every_cache_size(name, order):
    ref = reference_of(name)
    n_nodes = len(pu.get_case(name)["scene"]._np["nodes4"])
    assert n_nodes > 64                                # 64 is a real prefix
    for k in (0, 1, 2, 5, 21, 64):
        for lds_n in (1, -1):
            got, plan = trace(name, order, lds_n, k)
            assert plan[1] == k, (name, order, k, plan)
            assert plan[0] == 1 if lds_n == 1 else plan[0] >= 4
            for a, b in zip(got, ref):
                np.testing.assert_array_equal(a, b, f"{name} {order} k={k} lds_n={lds_n}")


def test_cached_walks_against_the_float64_reference():
    # the same walks against the brute-force reference, not only each other
    pu.check_walks("e_slab1500", device=0, lds_n=-1, n_cached=21)


_images = {}          # extra env (sorted tuple) -> accum array
_worker_failed = []   # first failing worker, if any


def render_with(tmp_path, extra_env):
    key = tuple(sorted(extra_env.items()))
    if key in _images:
        return _images[key]
    if _worker_failed:
        pytest.fail(f"not started: worker {_worker_failed[0]} failed before")
    env = {k: v for k, v in os.environ.items()
           if k not in ("HIPPT_TOPCACHE", "HIPPT_TOP_ORDER", "HIPPT_OCC")}
    env.update(extra_env)
    out = str(tmp_path / f"pt_{len(_images)}.npy")
    try:
        p = subprocess.run([sys.executable, WORKER, "pt", "4", out],
                           capture_output=True, text=True, timeout=90, env=env, cwd=ROOT)
    except subprocess.TimeoutExpired:
        _worker_failed.append(key)
        raise
    if p.returncode != 0:
        _worker_failed.append(key)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
    _images[key] = np.load(out)
    return _images[key]


@pytest.mark.parametrize("extra_env", [
    {},
    {"HIPPT_TOPCACHE": "0"},
    {"HIPPT_TOPCACHE": "1"},
    {"HIPPT_TOPCACHE": "21"},
    {"HIPPT_TOPCACHE": "256"},
], ids=["default", "cache0", "cache1", "cache21", "cache256"])
def test_pt_image_same_as_depth_first(tmp_path, extra_env):
    ref = render_with(tmp_path, {"HIPPT_TOP_ORDER": "dfs"})
    img = render_with(tmp_path, extra_env)
    assert ref.shape == (36, 64, 4) and np.isfinite(ref).all()
    assert float(ref[..., :3].mean()) > 1e-3 and (ref[..., 3] == 4).all()
    np.testing.assert_array_equal(img, ref)
