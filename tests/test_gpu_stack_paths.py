"""Device walks around the LDS / private boundary of the traversal stack
(csrc/core/bvh4.h: BVH_PUSH, BVH_POP under BVH_VISIT_TAGGED4's three pushes
of sorted (key, word) pairs and the any-hit visit's).  Neither the number of
LDS entries nor the node cache may change a result.

* Probe: Scene.trace_rays(device=0) with 1..6 LDS entries and with the
  launcher's own split, without and with 21 cached nodes.  The small values
  put the boundary inside ordinary walks and inside single visits, with
  lanes on both sides of it in one wave.  All five result arrays must equal
  the lds_n = 1, uncached run, and one setting is checked against the
  float64 brute force as well.
* Images: tests/occ_worker.py renders the small kitchen at the default, with
  the whole stack in scratch (HIPPT_STACK=scratch, lds_n = 0) and at
  HIPPT_OCC=6 HIPPT_TOPCACHE=256, which leaves four LDS entries.  One process
  per configuration under its own timeout; after the first worker that fails
  no further one is started.
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
SCENES = ["b_random400", "e_slab1500", "d_tris_spheres"]
LDS_N = [1, 2, 3, 4, 5, 6, -1]
CACHED = [0, 21]

_reference = {}   # case -> result arrays at lds_n = 1, n_cached = 0


def trace(name, lds_n, k):
    case = pu.get_case(name)
    scene = case["scene"]
    out = scene.trace_rays(case["o"], case["d"], case["tmax"], device=0, lds_n=lds_n,
                           n_cached=k)
    return out, scene.last_trace_plan


def reference_of(name):
    if name not in _reference:
        out, plan = trace(name, 1, 0)
        assert plan == (1, 0)
        assert (out[1] >= 0).sum() > 100               # the rays do hit
        assert out[4].any() and not out[4].all()       # some occluded, some not
        _reference[name] = out
    return _reference[name]


@pytest.mark.parametrize("k", CACHED)
@pytest.mark.parametrize("lds_n", LDS_N)
@pytest.mark.parametrize("name", SCENES)
def test_walks_same_at_every_stack_split(name, lds_n, k):
    ref = reference_of(name)
    assert len(pu.get_case(name)["scene"]._np["nodes4"]) > 21   # 21 is a real prefix
    got, plan = trace(name, lds_n, k)
    assert plan[1] == k, (name, lds_n, k, plan)
    assert plan[0] == lds_n if lds_n > 0 else plan[0] >= 4
    for a, b in zip(got, ref):
        np.testing.assert_array_equal(a, b, f"{name} lds_n={lds_n} k={k}")


def test_split_walks_against_the_float64_reference():
    # the same walks against the brute-force reference, not only each other
    pu.check_walks("e_slab1500", device=0, lds_n=3, n_cached=21)
    assert pu.get_case("e_slab1500")["scene"].last_trace_plan == (3, 21)


_images = {}          # extra env (sorted tuple) -> accum array
_worker_failed = []   # first failing worker, if any

STACK_ENV = ("HIPPT_TOPCACHE", "HIPPT_TOP_ORDER", "HIPPT_OCC", "HIPPT_STACK")


def render_with(tmp_path, extra_env):
    key = tuple(sorted(extra_env.items()))
    if key in _images:
        return _images[key]
    if _worker_failed:
        pytest.fail(f"not started: worker {_worker_failed[0]} failed before")
    env = {k: v for k, v in os.environ.items() if k not in STACK_ENV}
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
    {"HIPPT_STACK": "scratch"},
    {"HIPPT_OCC": "6", "HIPPT_TOPCACHE": "256"},
], ids=["scratch", "occ6_cache256"])
def test_pt_image_same_at_every_stack_split(tmp_path, extra_env):
    ref = render_with(tmp_path, {})
    img = render_with(tmp_path, extra_env)
    assert ref.shape == (36, 64, 4) and np.isfinite(ref).all()
    assert float(ref[..., :3].mean()) > 1e-3 and (ref[..., 3] == 4).all()
    np.testing.assert_array_equal(img, ref)
