"""GPU BVH4 walks vs the CPU integrator on scenes that exercise every branch
of the node phase: ordered closest-hit walks with 1-4 hit children per node
and multi-primitive leaves (kitchen depth), the triangle-only any-hit shadow
walk (kitchen pt) and the any-hit walk with spheres present (balls.xml).
Bounds are the ones test_gpu.py already uses for the same comparisons."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU visible", allow_module_level=True)

import hippt  # noqa: E402
from hippt.scene.procedural import kitchen  # noqa: E402
from hippt.scene.xml_parser import parse_xml  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pair(make_desc, spp):
    gpu = hippt.PythonRenderer(make_desc(), device_id=0).render(spp=spp).cpu().numpy()
    cpu = hippt.PythonRenderer(make_desc(), device_id=-1).render(spp=spp).numpy()
    return gpu, cpu


def test_kitchen_depth_matches_cpu():
    # every primary ray is one full ordered closest-hit walk; depth is
    # deterministic, so the bound is test_depth_deterministic's
    g, c = _pair(lambda: kitchen(width=160, height=90, renderer="depth"), spp=1)
    np.testing.assert_allclose(g[..., 0], c[..., 0], rtol=1e-3, atol=1e-3)


def test_kitchen_pt_matches_cpu():
    # triangle-only scene: closest-hit walk + any-hit shadow walk; bounds of
    # test_cornell_pt (measured at 4 spp: means 0.012% apart, 0.02% of pixels
    # more than 25% off, before and after the walk kept the node in registers)
    g, c = _pair(lambda: kitchen(width=160, height=90, renderer="pt"), spp=4)
    assert np.isfinite(g).all()
    gm, cm = g[..., :3].mean(), c[..., :3].mean()
    rel = np.abs(g[..., :3] - c[..., :3]) / (c[..., :3] + 0.05)
    print(f"kitchen pt: gpu mean {gm:.6f} cpu mean {cm:.6f} "
          f"rel {abs(gm - cm) / cm:.5f}, >25% off: {(rel > 0.25).mean():.4f}")
    assert abs(gm - cm) / cm < 0.02, (gm, cm)
    assert (rel > 0.25).mean() < 0.05, f"{(rel > 0.25).mean():.3f} of pixels diverge"


def test_balls_pt_matches_cpu():
    # spheres present: tri_only is off, the shadow walk reads the sphere bit
    def make():
        d = parse_xml(os.path.join(ROOT, "scenes", "balls.xml"))
        d.camera.width, d.camera.height = 96, 54
        return d
    g, c = _pair(make, spp=8)
    assert np.isfinite(g).all()
    m_gpu, m_cpu = g[..., :3].mean(), c[..., :3].mean()
    print(f"balls: gpu mean {m_gpu:.6f} cpu mean {m_cpu:.6f}")
    assert m_cpu > 0
    np.testing.assert_allclose(m_gpu, m_cpu, rtol=0.05)
