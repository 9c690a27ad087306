"""Small renders through the shading loaders (csrc/core/shade_load.h, the
LightPrim records of emitter.h), GPU against the CPU reference, pt and wfpt.

The scenes together reach every loader branch: sphere primitives, point light
and the light-selection CDF (balls.xml), area-spot light (spot-cbox.xml),
point light alone (point-cbox.xml), envmap (env-balls.xml), and, built in
tests/shade_util.py because no scene file has them, a sphere emitter and a
textured BSDF with a normal map and a roughness texture (spheres).

The comparison is the one of tests/test_gpu.py TestExampleScenesGPU._ab:
finite output and the GPU mean within rtol 0.05 of the CPU mean (the rtol
_ab uses for env-balls and point-cbox, and its default for the others).

Every GPU render is a child process with a time limit of its own
(tests/shade_worker.py); once one has failed no further one is started."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU visible", allow_module_level=True)

import hippt  # noqa: E402
from shade_worker import make_desc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "shade_worker.py")
W, H, SPP = 64, 36, 8
RTOL = 0.05
SCENES = ["balls", "spot-cbox", "point-cbox", "env-balls", "spheres"]

_cpu = {}
_failed = []


def cpu_reference(scene):
    """CPU image of a scene, rendered once and shared by pt and wfpt (the
    host runs one integrator for both)."""
    if scene not in _cpu:
        d = make_desc(scene, "pt", W, H)
        _cpu[scene] = hippt.PythonRenderer(d, device_id=-1).render(spp=SPP).numpy()
    return _cpu[scene]


def gpu_render(tmp_path, scene, renderer):
    if _failed:
        pytest.fail(f"not started: the render of {_failed[0]} failed before")
    out = str(tmp_path / "img.npy")
    try:
        p = subprocess.run([sys.executable, WORKER, scene, renderer, str(W), str(H),
                            str(SPP), out], capture_output=True, text=True,
                           timeout=120, cwd=ROOT)
    except subprocess.TimeoutExpired:
        _failed.append((scene, renderer))
        raise
    if p.returncode != 0:
        _failed.append((scene, renderer))
        pytest.fail(f"{scene}/{renderer}: exit {p.returncode}\n{p.stdout[-2000:]}\n"
                    f"{p.stderr[-2000:]}")
    return np.load(out)


@pytest.mark.parametrize("renderer", ["pt", "wfpt"])
@pytest.mark.parametrize("scene", SCENES)
def test_gpu_matches_cpu(tmp_path, scene, renderer):
    gpu = gpu_render(tmp_path, scene, renderer)
    cpu = cpu_reference(scene)
    assert gpu.shape == cpu.shape == (H, W, 4)
    assert np.isfinite(gpu).all(), scene
    m_gpu, m_cpu = gpu[..., :3].mean(), cpu[..., :3].mean()
    print(f"{scene}/{renderer}: gpu mean {m_gpu:.6f} cpu mean {m_cpu:.6f} "
          f"rel {abs(m_gpu - m_cpu) / m_cpu:.5f}")
    assert m_cpu > 0
    np.testing.assert_allclose(m_gpu, m_cpu, rtol=RTOL, err_msg=f"{scene}/{renderer}")
