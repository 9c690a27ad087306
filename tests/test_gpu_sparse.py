"""Brick-layout grid media on the device: k_render<R_VOLUME_PT> with the
two-load brick lookup vs the dense lookup.  GPU runs are deterministic
(TestGPUDeterminism) and both layouts load the same voxel values into the
same arithmetic, so sparse == dense is asserted exactly."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU visible", allow_module_level=True)

import hippt  # noqa: E402
from hippt.scene.procedural import smoke_box, sparse_smoke_box  # noqa: E402
from hippt.scene.scene import MediumDesc  # noqa: E402
from hippt.scene.sparse_grid import SparseGrid  # noqa: E402


def random_brick_grid(shape, empty_frac=0.7, seed=11):
    rng = np.random.default_rng(seed)
    nz, ny, nx = shape
    bz, by, bx = (-(-nz // 8), -(-ny // 8), -(-nx // 8))
    keep = rng.random((bz, by, bx)) >= empty_frac
    keep.flat[0] = True
    mask = np.repeat(np.repeat(np.repeat(keep, 8, 0), 8, 1), 8, 2)[:nz, :ny, :nx]
    a = rng.random(shape).astype(np.float32) * mask
    a[rng.random(shape) < 0.3] = 0.0
    return a.astype(np.float32)


def hand_built(density, width, height):
    d = smoke_box(width=width, height=height, n_grid=8)
    d.media = [MediumDesc(type="grid", sigma_a=(0.3, 0.35, 0.4), sigma_s=(2.5, 2.5, 2.5),
                          phase="hg", g1=0.2, density=density, scale=6.0,
                          grid_lo=(-0.7, 0.05, 0.5), grid_hi=(0.7, 1.75, 1.9))]
    return d


def sparsified(desc):
    m = desc.media[0]
    m.density = SparseGrid.from_dense(m.density)
    return desc


def render(desc, spp, device=0):
    r = hippt.PythonRenderer(desc, device_id=device)
    img = r.render(spp=spp)
    img = img.cpu().numpy() if device >= 0 else img.numpy().copy()
    info = r.info()
    r.release()
    return img, info


@pytest.fixture(scope="module")
def smoke_pair():
    """smoke_box 96x54 n_grid=48 at 8 spp on device 0, dense and bricks."""
    dense, di = render(smoke_box(width=96, height=54, n_grid=48), 8)
    bricks, bi = render(sparsified(smoke_box(width=96, height=54, n_grid=48)), 8)
    return dense, di, bricks, bi


def test_smoke_box_bricks_equal_dense(smoke_pair):
    dense, di, bricks, bi = smoke_pair
    assert di["media"][0]["layout"] == "dense" and bi["media"][0]["layout"] == "bricks"
    assert bi["media"][0]["bytes_device"] == bi["media"][0]["bytes_host"] > 0
    assert np.isfinite(dense).all() and dense[..., :3].mean() > 0
    np.testing.assert_array_equal(bricks, dense)


def test_smoke_box_emission_bricks_equal_dense():
    dense, _ = render(smoke_box(width=96, height=54, n_grid=48, emission=True), 8)
    bricks, _ = render(sparsified(smoke_box(width=96, height=54, n_grid=48, emission=True)), 8)
    np.testing.assert_array_equal(bricks, dense)


def test_odd_grid_bricks_equal_dense():
    a = random_brick_grid((17, 40, 24))
    dense, _ = render(hand_built(a, 96, 54), 8)
    bricks, _ = render(hand_built(SparseGrid.from_dense(a), 96, 54), 8)
    assert dense[..., :3].mean() > 0
    np.testing.assert_array_equal(bricks, dense)


def test_dense_medium_through_brick_kernel(smoke_pair):
    """A scene holding any brick medium runs the kernel instantiation with
    the layout test; its dense media must render as the dense-only kernel
    renders them.  The extra brick medium here is referenced by no object."""
    d = smoke_box(width=96, height=54, n_grid=48)
    d.media.append(MediumDesc(type="grid", density=SparseGrid.from_dense(
        random_brick_grid((17, 40, 24)))))
    img, info = render(d, 8)
    assert [m["layout"] for m in info["media"]] == ["dense", "bricks"]
    np.testing.assert_array_equal(img, smoke_pair[0])


def test_gpu_sparse_vs_cpu_sparse(smoke_pair):
    g = smoke_pair[2]
    c, _ = render(sparsified(smoke_box(width=96, height=54, n_grid=48)), 8, device=-1)
    gm, cm = g[..., :3].mean(), c[..., :3].mean()
    assert np.isfinite(g).all()
    assert abs(gm - cm) / cm < 0.05, (gm, cm)


def test_large_sparse_scene():
    img, info = render(sparse_smoke_box(width=96, height=54, n_grid=512), 4)
    assert np.isfinite(img).all() and img[..., :3].mean() > 0
    mi = info["media"][0]
    assert mi["layout"] == "bricks" and mi["shape"] == (512, 512, 512)
    assert mi["bytes_dense_equiv"] == 4 * 512 ** 3
    assert 0 < mi["bytes_device"] < 0.05 * mi["bytes_dense_equiv"], mi


@pytest.mark.parametrize("case", ["partial", "empty", "full"])
def test_edge_shapes(case):
    if case == "partial":
        a = np.arange(1, 31, dtype=np.float32).reshape(2, 3, 5) / 30.0
    elif case == "empty":
        a = np.zeros((17, 40, 24), np.float32)
    else:
        a = np.random.default_rng(2).random((16, 16, 16)).astype(np.float32) + 0.5
    g = SparseGrid.from_dense(a)
    assert g.n_bricks == {"partial": 1, "empty": 0, "full": 8}[case]
    dense, _ = render(hand_built(a, 32, 24), 2)
    bricks, bi = render(hand_built(g, 32, 24), 2)
    assert bi["media"][0]["n_bricks"] == g.n_bricks
    assert np.isfinite(bricks).all()
    np.testing.assert_array_equal(bricks, dense)


def test_hot_reload_scale_on_device():
    imgs = []
    for sparse in (False, True):
        d = smoke_box(width=96, height=54, n_grid=48)
        if sparse:
            sparsified(d)
        r = hippt.PythonRenderer(d, device_id=0)
        before = r.render(spp=2).cpu().numpy()
        r.scene.set_medium(0, scale=0.25)
        r.reset()
        after = r.render(spp=2).cpu().numpy()
        assert not np.array_equal(before, after)
        imgs.append(after)
        r.release()
    np.testing.assert_array_equal(imgs[1], imgs[0])
