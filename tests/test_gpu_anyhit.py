"""Device side of tests/test_anyhit_host.py: the any-hit walk and the leaf
loops that read the whole primitive first (one wait per primitive), in the
wavefront kernels' LDS layout against the float64 brute force of
tests/probe_util.py, and the NEE path end to end against the CPU render.

(lds_n, n_cached): the launcher's own plan, and one and three stack entries
in LDS with no cached tree top, so that the three unrolled pushes of a visit
cross from LDS into private memory at different positions.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU visible", allow_module_level=True)

import hippt  # noqa: E402
import probe_util as pu  # noqa: E402
import test_anyhit_host as ta  # noqa: E402,F401  (registers the f_tris5 case)
from hippt.scene.procedural import cornell_box  # noqa: E402

PLANS = [(-1, -1), (1, 0), (3, 0)]


@pytest.mark.parametrize("lds_n,n_cached", PLANS)
@pytest.mark.parametrize("name", ["a_single", "f_tris5", "b_random400",
                                  "d_tris_spheres", "e_slab1500"])
def test_device_walks(name, lds_n, n_cached):
    pu.check_walks(name, device=0, lds_n=lds_n, n_cached=n_cached)
    if lds_n >= 0:
        assert pu.get_case(name)["scene"].last_trace_plan == (lds_n, n_cached)


def test_cornell_pt_matches_cpu():
    # every bounce casts a shadow ray at the area light: the any-hit walk end
    # to end.  Comparison and bounds of tests/test_gpu_walk.py's pt render.
    def make():
        return cornell_box(width=64, height=64, renderer="pt")
    g = hippt.PythonRenderer(make(), device_id=0).render(spp=4).cpu().numpy()
    c = hippt.PythonRenderer(make(), device_id=-1).render(spp=4).numpy()
    assert np.isfinite(g).all()
    gm, cm = g[..., :3].mean(), c[..., :3].mean()
    rel = np.abs(g[..., :3] - c[..., :3]) / (c[..., :3] + 0.05)
    print(f"cornell pt: gpu mean {gm:.6f} cpu mean {cm:.6f} "
          f"rel {abs(gm - cm) / cm:.5f}, >25% off: {(rel > 0.25).mean():.4f}")
    assert abs(gm - cm) / cm < 0.02, (gm, cm)
    assert (rel > 0.25).mean() < 0.05, f"{(rel > 0.25).mean():.3f} of pixels diverge"
