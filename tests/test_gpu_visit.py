"""Device side of tests/test_visit_host.py: the tagged-node walks on a tree
with empty slots and one internal child, and every occupancy instantiation
of the megakernels.

HIPPT_OCC picks the k_render instantiation (waves/SIMD pin) and the LDS
budget, i.e. how many stack entries sit in LDS and how many in private
memory; it must not change a single bit of the image.  The knob is read at
the first launch, so every value renders in a process of its own
(tests/occ_worker.py), each under its own timeout; after the first worker
that exits non-zero no further one is started.  One more worker asks for a
top-tree cache larger than its occupancy's LDS budget holds.
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
import test_visit_host as tv  # noqa: E402,F401  (registers the f_tris5 case)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "occ_worker.py")


@pytest.mark.parametrize("lds_n,n_cached", [(0, 0), (1, 1), (-1, -1)])
def test_device_walks_five_triangles(lds_n, n_cached):
    pu.check_walks("f_tris5", device=0, lds_n=lds_n, n_cached=n_cached)
    used_lds, used_cache = pu.get_case("f_tris5")["scene"].last_trace_plan
    if lds_n >= 0:
        assert (used_lds, used_cache) == (lds_n, n_cached)
    else:
        assert used_lds >= 4 and used_cache == 2     # the whole two-node tree


_images = {}          # (renderer, occ, extra env) -> accum array
_worker_failed = []   # first failing worker, if any


def render_at(tmp_path, renderer, spp, occ, extra_env=None):
    extra_env = extra_env or {}
    key = (renderer, occ, tuple(sorted(extra_env.items())))
    if key in _images:
        return _images[key]
    if _worker_failed:
        pytest.fail(f"not started: worker {_worker_failed[0]} failed before")
    env = {k: v for k, v in os.environ.items() if k != "HIPPT_OCC"}
    if occ is not None:
        env["HIPPT_OCC"] = str(occ)
    env.update(extra_env)
    out = str(tmp_path / f"{renderer}_{occ}_{len(_images)}.npy")
    try:
        p = subprocess.run([sys.executable, WORKER, renderer, str(spp), out],
                           capture_output=True, text=True, timeout=90, env=env, cwd=ROOT)
    except subprocess.TimeoutExpired:
        _worker_failed.append(key)
        raise
    if p.returncode != 0:
        _worker_failed.append(key)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
    _images[key] = np.load(out)
    return _images[key]


def check_same_image(tmp_path, renderer, spp, occ, extra_env=None):
    ref = render_at(tmp_path, renderer, spp, None)
    img = render_at(tmp_path, renderer, spp, occ, extra_env)
    assert ref.shape == (36, 64, 4) and np.isfinite(ref).all()
    assert float(ref[..., :3].mean()) > 1e-3 and (ref[..., 3] == spp).all()
    np.testing.assert_array_equal(img, ref)


@pytest.mark.parametrize("occ", [3, 4, 5, 6, 8])
def test_pt_image_same_at_every_occupancy(tmp_path, occ):
    check_same_image(tmp_path, "pt", 4, occ)


@pytest.mark.parametrize("occ", [4, 6])
def test_vpt_image_same_at_every_occupancy(tmp_path, occ):
    check_same_image(tmp_path, "vpt", 2, occ)


def test_pt_image_same_with_cache_request_above_the_budget(tmp_path):
    # 256 nodes do not fit beside 4 stack entries in the 12-entry budget of
    # occupancy 6: the plan cuts the cache to 128 (tests/test_lds_plan.py)
    check_same_image(tmp_path, "pt", 4, 6, {"HIPPT_TOPCACHE": "256"})
