"""Scene.shade_probe on the device (k_shade_probe, the shading loaders of
csrc/core/shade_load.h with their asm statement) against the scene's tables
and against the host probe, exactly: the records are loaded data."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU visible", allow_module_level=True)

import shade_util as su  # noqa: E402


@pytest.mark.parametrize("name", ["cornell", "spheres", "no_emitter", "shared_bsdf"])
def test_device_probe_matches_tables_and_host(name):
    scene = su.get_scene(name)
    q, kinds, dev = su.check_probe(scene, device=0)
    host = scene.shade_probe(q, device=-1)
    for d, h in zip(dev, host):
        np.testing.assert_array_equal(d, h)
    if name == "spheres":
        assert np.isin(q, kinds["sph"]).any() and np.isin(q, kinds["em"]).any()
