"""GPU kernel tests: HIP megakernels vs the CPU reference integrator (same
single-source core, same RNG streams), run on a real MI355X via gpurun."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU visible", allow_module_level=True)

import hippt  # noqa: E402
from hippt.scene.procedural import cornell_box, kitchen, smoke_box, sports_car  # noqa: E402


def test_native_extension_in_tree():
    assert "/hippt/" in hippt.C.__file__.replace("\\", "/")


def render_pair(desc_fn, spp=16, **kw):
    d_gpu = desc_fn(**kw)
    r_gpu = hippt.PythonRenderer(d_gpu, device_id=0)
    img_gpu = r_gpu.render(spp=spp).cpu().numpy()
    d_cpu = desc_fn(**kw)
    r_cpu = hippt.PythonRenderer(d_cpu, device_id=-1)
    img_cpu = r_cpu.render(spp=spp).numpy()
    return img_gpu, img_cpu


class TestNumericsVsCPU:
    def test_cornell_pt(self):
        g, c = render_pair(cornell_box, spp=16, width=96, height=96, max_depth=5)
        gm, cm = g[..., :3].mean(), c[..., :3].mean()
        assert abs(gm - cm) / cm < 0.02, (gm, cm)
        # most pixels should agree closely (same RNG streams; fp divergence
        # can flip individual RR decisions)
        rel = np.abs(g[..., :3] - c[..., :3]) / (c[..., :3] + 0.05)
        assert (rel > 0.25).mean() < 0.05, f"{(rel > 0.25).mean():.3f} of pixels diverge"

    def test_depth_deterministic(self):
        g, c = render_pair(cornell_box, spp=4, width=64, height=64, renderer="depth")
        np.testing.assert_allclose(g[..., 0], c[..., 0], rtol=1e-3, atol=1e-3)

    def test_vpt_smoke(self):
        g, c = render_pair(smoke_box, spp=8, width=96, height=54, n_grid=48)
        gm, cm = g[..., :3].mean(), c[..., :3].mean()
        assert np.isfinite(g).all()
        assert abs(gm - cm) / cm < 0.05, (gm, cm)

    def test_light_tracer(self):
        d = cornell_box(width=64, height=64, renderer="lt", max_depth=5)
        r = hippt.PythonRenderer(d, device_id=0)
        img = r.render(spp=16).cpu().numpy()
        assert np.isfinite(img).all()
        assert img[..., :3].mean() > 0.01
        # LT and PT estimate the same integral
        d2 = cornell_box(width=64, height=64, renderer="pt", max_depth=5)
        pt = hippt.PythonRenderer(d2, device_id=0).render(spp=32).cpu().numpy()
        ratio = img[..., :3].mean() / pt[..., :3].mean()
        assert 0.7 < ratio < 1.3, ratio


class TestBigScenes:
    def test_kitchen_renders(self):
        d = kitchen(width=480, height=270)
        r = hippt.PythonRenderer(d, device_id=0)
        img = r.render(spp=4).cpu().numpy()
        assert np.isfinite(img).all()
        assert img[..., :3].mean() > 0.01
        assert r.info()["n_prims"] > 50000

    def test_sports_car_renders(self):
        d = sports_car(width=480, height=270)
        r = hippt.PythonRenderer(d, device_id=0)
        img = r.render(spp=4).cpu().numpy()
        assert np.isfinite(img).all()
        assert img[..., :3].mean() > 0.005


class TestGPUDeterminism:
    def test_same_seed_same_image(self):
        d = cornell_box(width=64, height=64, max_depth=4)
        a = hippt.PythonRenderer(d, device_id=0).render(spp=8).cpu().numpy()
        d2 = cornell_box(width=64, height=64, max_depth=4)
        b = hippt.PythonRenderer(d2, device_id=0).render(spp=8).cpu().numpy()
        np.testing.assert_array_equal(a, b)


class TestWavefront:
    def test_wfpt_matches_megakernel(self):
        d = cornell_box(width=96, height=96, max_depth=5, renderer="wfpt")
        wf = hippt.PythonRenderer(d, device_id=0).render(spp=24).cpu().numpy()
        d2 = cornell_box(width=96, height=96, max_depth=5, renderer="pt")
        mk = hippt.PythonRenderer(d2, device_id=0).render(spp=24).cpu().numpy()
        assert np.isfinite(wf).all()
        m1, m2 = wf[..., :3].mean(), mk[..., :3].mean()
        assert abs(m1 - m2) / m2 < 0.03, (m1, m2)
        # structural agreement (both estimate the same integral)
        diff = np.abs(wf[..., :3] - mk[..., :3]).mean()
        assert diff < 0.25 * m2 + 0.05, diff

    def test_wfpt_kitchen(self):
        d = kitchen(width=480, height=270, renderer="wfpt")
        r = hippt.PythonRenderer(d, device_id=0)
        img = r.render(spp=4).cpu().numpy()
        assert np.isfinite(img).all()
        assert img[..., :3].mean() > 0.01


class TestVariants:
    def test_pt_dyn_matches_pt(self):
        d = cornell_box(width=64, height=64, max_depth=4, renderer="pt-dyn")
        dyn = hippt.PythonRenderer(d, device_id=0).render(spp=16).cpu().numpy()
        d2 = cornell_box(width=64, height=64, max_depth=4, renderer="pt")
        st = hippt.PythonRenderer(d2, device_id=0).render(spp=16).cpu().numpy()
        # identical sampler streams -> near-identical images
        np.testing.assert_allclose(dyn[..., :3].mean(), st[..., :3].mean(), rtol=0.01)

    def test_sbvh_matches_bvh(self):
        d = kitchen(width=160, height=90)
        d.config.use_sbvh = True
        sb = hippt.PythonRenderer(d, device_id=0).render(spp=4).cpu().numpy()
        d2 = kitchen(width=160, height=90)
        bv = hippt.PythonRenderer(d2, device_id=0).render(spp=4).cpu().numpy()
        np.testing.assert_allclose(sb[..., :3].mean(), bv[..., :3].mean(), rtol=0.01)

    def test_xml_scene_on_gpu(self):
        import os
        from hippt.scene.xml_parser import parse_xml
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        d = parse_xml(os.path.join(root, "scenes", "balls.xml"))
        d.camera.width, d.camera.height = 160, 90
        img = hippt.PythonRenderer(d, device_id=0).render(spp=8).cpu().numpy()
        assert np.isfinite(img).all()
        assert img[..., :3].mean() > 0.01

    def test_hot_reload_on_gpu(self):
        d = cornell_box(width=48, height=48, max_depth=4)
        r = hippt.PythonRenderer(d, device_id=0)
        a = r.render(spp=8).cpu().numpy()
        from hippt.scene.scene import BsdfDesc
        r.scene.set_bsdf(1, BsdfDesc(type="specular"))   # red wall -> mirror
        r.reset()
        b = r.render(spp=8).cpu().numpy()
        assert abs(a[..., 0].mean() - b[..., 0].mean()) > 1e-3

    def test_bdpt_mode(self):
        d = cornell_box(width=48, height=48, max_depth=4, renderer="bdpt")
        img = hippt.PythonRenderer(d, device_id=0).render(spp=8).cpu().numpy()
        assert np.isfinite(img).all()
        assert img[..., :3].mean() > 0.01


@pytest.mark.gpu
class TestExampleScenesGPU:
    """Each shipped example XML renders on the GPU and agrees with the CPU
    reference path in mean brightness (same sampler streams)."""

    def _ab(self, name, spp=8, w=96, h=96, rtol=0.05):
        import os
        from hippt.scene.xml_parser import parse_xml
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        d = parse_xml(os.path.join(root, "scenes", name))
        d.camera.width, d.camera.height = w, h
        gpu = hippt.PythonRenderer(d, device_id=0).render(spp=spp).cpu().numpy()
        d2 = parse_xml(os.path.join(root, "scenes", name))
        d2.camera.width, d2.camera.height = w, h
        cpu = hippt.PythonRenderer(d2, device_id=-1).render(spp=spp).numpy()
        assert np.isfinite(gpu).all(), name
        m_gpu, m_cpu = gpu[..., :3].mean(), cpu[..., :3].mean()
        assert m_cpu > 0
        np.testing.assert_allclose(m_gpu, m_cpu, rtol=rtol, err_msg=name)

    def test_grid_cbox(self):
        self._ab("grid-cbox.xml")

    def test_tof_cbox(self):
        self._ab("tof-cbox.xml", spp=16, rtol=0.1)

    def test_diamonds(self):
        self._ab("diamonds.xml", w=96, h=54, rtol=0.1)

    def test_env_balls(self):
        self._ab("env-balls.xml", w=96, h=54)

    def test_caustics_lt(self):
        self._ab("caustics-lt.xml", spp=32, rtol=0.2)

    def test_point_cbox(self):
        self._ab("point-cbox.xml")


@pytest.mark.gpu
def test_adaptive_sampling_gpu():
    d = cornell_box(width=64, height=64, max_depth=4)
    r = hippt.PythonRenderer(d, device_id=0)
    img = r.render(spp=32, adaptive=True).cpu().numpy()
    assert np.isfinite(img).all()
    cnt = img[..., 3]
    assert cnt.std() > 0.5 and cnt.min() >= 8
    d2 = cornell_box(width=64, height=64, max_depth=4)
    u = hippt.PythonRenderer(d2, device_id=0).render(spp=32).cpu().numpy()
    assert abs(img[..., :3].mean() - u[..., :3].mean()) < 0.05 * u[..., :3].mean()


@pytest.mark.gpu
def test_denoiser_gpu():
    d = cornell_box(width=96, height=96, max_depth=4)
    r = hippt.PythonRenderer(d, device_id=0)
    r.renderer.enable_aov()
    r.render(spp=8)
    den = r.renderer.denoise()
    assert den.is_cuda and torch.isfinite(den).all()
    d2 = cornell_box(width=96, height=96, max_depth=4)
    ref = hippt.PythonRenderer(d2, device_id=0, seed_offset=3).render(spp=512).cpu().numpy()[..., :3]
    noisy = r.renderer.raw()[..., :3].cpu().numpy()
    dn = den.cpu().numpy()
    crop = np.s_[30:84, 12:84]
    rn = float(np.sqrt(((noisy[crop] - ref[crop]) ** 2).mean()))
    rd = float(np.sqrt(((dn[crop] - ref[crop]) ** 2).mean()))
    assert rd < 0.6 * rn, (rd, rn)


@pytest.mark.gpu
def test_band_render_exact():
    """Tile-band rendering (y0/y1) composes exactly: two half-band renders
    accumulate to the same buffer as one full render (same per-pixel sampler
    streams; disjoint rows)."""
    d = cornell_box(width=64, height=64, max_depth=4)
    r_full = hippt.PythonRenderer(d, device_id=0)
    r_full.renderer.render(8)
    full = r_full.renderer.accum.cpu().numpy()
    d2 = cornell_box(width=64, height=64, max_depth=4)
    r_band = hippt.PythonRenderer(d2, device_id=0)
    r_band.renderer.render(8, y0=0, y1=32)
    r_band.renderer.accum_cnt -= 8   # same sample indices for the second band
    r_band.renderer.render(8, y0=32, y1=64)
    band = r_band.renderer.accum.cpu().numpy()
    np.testing.assert_array_equal(full, band)


@pytest.mark.gpu
def test_renderer_scene_matrix():
    """Every renderer on every applicable scene: finite, non-black output."""
    from hippt.scene.procedural import cornell_box, kitchen, smoke_box
    combos = []
    for kind in ["pt", "pt-dyn", "wfpt", "vpt", "lt", "bdpt", "depth", "bvh-cost"]:
        combos.append(("cornell", cornell_box(width=64, height=64, max_depth=4,
                                              renderer=kind), kind))
    for kind in ["pt", "wfpt", "vpt", "depth"]:
        d = kitchen(width=96, height=54, detail=0.25)
        d.config.renderer = kind
        combos.append(("kitchen", d, kind))
    for kind in ["vpt", "pt"]:
        d = smoke_box(width=64, height=48, n_grid=24)
        d.config.renderer = kind
        combos.append(("smoke", d, kind))
    for name, d, kind in combos:
        r = hippt.PythonRenderer(d, device_id=0)
        img = r.render(spp=4).cpu().numpy()
        assert np.isfinite(img).all(), (name, kind)
        assert img[..., :3].max() > 0, (name, kind)
        r.release()


def test_two_rank_ddp_smoke_single_gpu():
    """DDP code path with 2 ranks sharing one GPU: rendering runs on cuda:0
    in both ranks, the spp-weighted all-reduce runs over gloo host copies
    (RCCL refuses duplicate devices).  Validates the multi-rank bench path
    end-to-end on hardware; true RCCL/xGMI scaling is the driver's 8-GPU
    SCALE run."""
    import json
    import os
    import subprocess
    import sys
    env = dict(os.environ, HIPPT_DDP_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29871", "bench.py", "--gpus", "2", "--steps", "2",
         "--warmup", "1", "--width", "480", "--height", "270",
         "--spp-per-step", "4"],
        capture_output=True, text=True, timeout=300, env=env,
        cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    assert d["n_gpus"] == 2 and d["value"] > 0, d


def test_envmap_light_tracing_gpu():
    """Envmap sample_le on the HIP path: light tracing an env-lit sphere
    must agree with PT (round-2 feature; CPU counterpart in
    tests/test_render_cpu.py)."""
    from hippt.scene.scene import (SceneDesc, ObjectDesc, BsdfDesc, EmitterDesc,
                                   CameraDesc, RenderConfig)
    sun = np.full((32, 64, 4), 0.08, np.float32)
    sun[4:10, 12:20, :3] = 25.0

    def scene(renderer):
        d = SceneDesc()
        d.textures = [sun.copy()]
        d.bsdfs = [BsdfDesc(type="lambertian", kd=(0.65, 0.6, 0.55))]
        d.emitters = [EmitterDesc(type="envmap", emission=(1, 1, 1), scale=1.0,
                                  tex_id=0)]
        d.objects = [ObjectDesc(spheres=np.array([[0, 0, 0, 1.0]], np.float32),
                                bsdf=0)]
        d.camera = CameraDesc(pos=(0, 0, -4), lookat=(0, 0, 0), fov=35,
                              width=64, height=64)
        d.config = RenderConfig(renderer=renderer, spp=1, max_depth=5)
        return d

    lt = hippt.PythonRenderer(scene("lt"), device_id=0).render(spp=128).cpu().numpy()
    pt = hippt.PythonRenderer(scene("pt"), device_id=0).render(spp=128).cpu().numpy()
    lt_c = lt[22:42, 22:42, :3].mean()
    pt_c = pt[22:42, 22:42, :3].mean()
    assert lt_c > 1e-3, "GPU LT from envmap produced a black image"
    assert abs(lt_c - pt_c) < 0.25 * pt_c, (lt_c, pt_c)


def test_wavefront_split_pipeline_env():
    """The classic per-bounce split pipeline (HIPPT_WF_FUSE=0: shade /
    shadow-queue / trace kernels + per-bounce sort) stays correct — it is
    the measured A/B baseline for the fused-span design.  Env is read at
    first launch, so run in a subprocess.  HIPPT_WF_TAIL=0 keeps the tail
    kernel from taking every path over after the first sort (the default
    threshold is far above this frame), and the [wf] log must show one sort
    per stage: kitchen's max_depth is 10, so bounces 0..10, the last of
    which finds no live ray (a path ends once it has bounced max_depth
    times, as in the megakernel)."""
    import os
    import re
    import subprocess
    import sys
    code = (
        "import hippt, numpy as np\n"
        "from hippt.scene.procedural import kitchen\n"
        "d = kitchen(width=192, height=108, renderer='wfpt')\n"
        "r = hippt.PythonRenderer(d, device_id=0)\n"
        "img = r.render(spp=8).cpu().numpy()\n"
        "assert np.isfinite(img).all() and img[..., :3].mean() > 0.01\n"
        "d2 = kitchen(width=192, height=108, renderer='pt')\n"
        "p = hippt.PythonRenderer(d2, device_id=0).render(spp=8).cpu().numpy()\n"
        "ratio = img[..., :3].mean() / p[..., :3].mean()\n"
        "assert 0.9 < ratio < 1.1, ratio\n"
        "print('split ok', ratio)\n")
    env = dict(os.environ, HIPPT_WF_FUSE="0", HIPPT_WF_SPAN="1",
               HIPPT_WF_TAIL="0", HIPPT_WF_LOG="1")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True,
                         text=True, timeout=240, env=env,
                         cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-1500:]
    assert "split ok" in out.stdout
    lines = [(int(b), int(n)) for b, n in
             re.findall(r"^\[wf\] spp 0 bounce (\d+) live (\d+)", out.stdout, re.M)]
    assert [b for b, _ in lines] == list(range(11)), lines
    live = [n for _, n in lines]
    assert all(0 < n <= 192 * 108 for n in live[:10]) and live[10] == 0, live
    assert all(a >= b for a, b in zip(live, live[1:])), live


def test_xml_scenes_on_gpu():
    """XML-driven paths on HIP that the procedural GPU tests miss:
    spectral dispersion (diamonds), multi-material OBJ hero (.mtl-derived
    GGX/glass/textures), and the NanoVDB grid medium."""
    import os
    from hippt.scene.xml_parser import parse_xml
    root = os.path.join(os.path.dirname(__file__), "..", "scenes")
    for name, min_mean in [("diamonds", 0.01), ("hero", 0.01),
                           ("grid-cbox-nvdb", 0.01)]:
        d = parse_xml(os.path.join(root, name + ".xml"))
        d.camera.width, d.camera.height = 96, 54
        r = hippt.PythonRenderer(d, device_id=0)
        img = r.render(spp=8).cpu().numpy()
        assert np.isfinite(img).all(), name
        assert img[..., :3].mean() > min_mean, (name, img[..., :3].mean())
        r.release()
