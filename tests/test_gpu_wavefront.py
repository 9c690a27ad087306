"""The wavefront pipeline behind the tail handoff.  launch_render_wavefront
hands every surviving path to k_wf_tail once `live <= HIPPT_WF_TAIL` (default
1 536 000 rays), so at test sizes nothing after the first sort runs unless
HIPPT_WF_TAIL=0.  Every configuration here renders in a child process of its
own (tests/wf_worker.py; the launcher reads its env hooks once per process)
with HIPPT_WF_TAIL=0 and HIPPT_WF_LOG=1, and is compared with the megakernel
and the CPU render of the same scene, spp and seed.

Measured on an MI355X.  No configuration is bit-identical to the megakernel
(the kernels are compiled separately), so none asserts array_equal; but the
differences are rounding-sized except where a Russian-roulette or hit
decision flips (kitchen).  Columns: accumulator values that differ from the
megakernel's / largest |difference| of the spp-sums; rel = relative
difference of the image means, off = share of values with
|a-b|/(b+0.05) > 0.25 (bounds 2 % and 5 %), against the megakernel and
against the CPU render; live = the [wf] live counts.

  config              differ        max|d|   mk rel   mk off  cpu rel   cpu off  live
  span2               774/36864     2.6e-6   0        0       0         0        5652 3621
  span1               877/36864     2.6e-6   0        0       0         0        6991 5652 4533 3621 0
  span3_last_cnt1     744/36864     2.6e-6   0        0       0         0        4533 0
  span8_default       830/36864     2.6e-6   0        0       0         0        723
  span3_last_notrace  737/36864     2.6e-6   0        0       0         0        4533
  span2_compact       774/36864     2.6e-6   0        0       0         0        5652 3621
  span2_raygen        774/36864     2.6e-6   0        0       0         0        9216 5652 3621
  kitchen_span2       6104/57600    2.4e-2   4.5e-5%  0       0.0123%   0.0185%  14357 14281 13577 5772 0
  env_balls_span2     1395/20736    7.6e-6   0        0       1.0e-5%   0        1079 453 0
  ("0" = below 1e-7 %.)  The kitchen figures against the CPU are the ones
  tests/test_gpu_walk.py records for the megakernel itself.

  split, split_dual: D = 1.8e-7 against D_ref = 0.0884 (bound 0.1767); image
  mean difference 0 against a largest pairwise difference of 1.73e-3 (bound
  3.47e-3, mean 0.7822); 1370 of 16384 values differ from the megakernel's.
  k_wf_shade in fact draws its random numbers in the integrator's order;
  the test does not rely on it.  live 4096 3079 2477 1990 1587 0.

The stage at bounce == max_depth.  The launcher's loop runs to max_depth + 1
stages, but a path ends once it has bounced max_depth times (path_step's
entry cap, k_wf_shade's `nb >= max_depth`), exactly as in the megakernel.  A
sort that lands on bounce == max_depth therefore finds no live ray in a
scene without null-lobe materials, and no kernel follows it: a "last step
with cnt=1, do_trace=0" on live rays cannot happen.  check_log asserts that
count to be exactly 0 (a live ray there would be a shade the megakernel never
does) and every earlier count to be positive; span3_last_notrace adds the
case in which the last step does run on live rays with do_trace=0.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU visible", allow_module_level=True)

import hippt  # noqa: E402
from hippt import C  # noqa: E402
from wf_worker import make_desc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "wf_worker.py")
WF_LINE = re.compile(r"^\[wf\] spp 0 bounce (\d+) live (\d+)", re.M)
DEFAULT_SPAN = 8


def expected_sorts(n_stage, span=DEFAULT_SPAN, fuse=True, primary_fuse=True):
    """Bounce indices at which launch_render_wavefront sorts: the primary
    kernel covers the first `span` shades when fused, then one sort per
    `span` shades (fused) or per shade (split) up to max_depth + 1 shades."""
    first = min(span, n_stage) if (fuse and primary_fuse) else 0
    return list(range(first, n_stage, span if fuse else 1))


def run_worker(tmp_path, scene, w, h, spp, max_depth, env):
    out = str(tmp_path / "accum.npy")
    full = {k: v for k, v in os.environ.items() if not k.startswith("HIPPT_WF_")}
    full.update(env, HIPPT_WF_TAIL="0", HIPPT_WF_LOG="1")
    p = subprocess.run([sys.executable, WORKER, scene, str(w), str(h), str(spp),
                        str(max_depth), out], capture_output=True, text=True,
                       timeout=120, env=full, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
    lines = [(int(b), int(n)) for b, n in WF_LINE.findall(p.stdout)]
    return np.load(out), lines


def check_log(lines, expect_bounces, n_pix, max_depth):
    """One [wf] line per sort of the launcher's loop, live counts in
    (0, w*h] and never increasing.  The loop runs to max_depth + 1 stages,
    but the integrator ends a path once it has bounced max_depth times
    (path_step's entry cap; null-lobe bounces, which none of these scenes
    has, do not count), as the megakernel does.  So a sort that lands on
    bounce == max_depth must find NO live ray — one more would be a shade
    the megakernel never does — and every earlier sort must find some."""
    assert [b for b, _ in lines] == expect_bounces, (lines, expect_bounces)
    live = [n for _, n in lines]
    assert all(0 < n <= n_pix for b, n in lines if b < max_depth), lines
    assert all(n == 0 for b, n in lines if b >= max_depth), lines
    assert all(a >= b for a, b in zip(live, live[1:])), live


_REFS = {}


def references(scene, w, h, spp, max_depth, seeds=(0,), cpu=True, shallower=False):
    """Megakernel accumulation buffers per seed_offset (GPU) and the CPU
    render (seed 0), rendered once per module for each scene setup;
    `shallower` adds the megakernel at max_depth - 1 (seed 0)."""
    key = (scene, w, h, spp, max_depth)
    ref = _REFS.setdefault(key, {"mk": {}, "cpu": None, "mk_shallow": None})
    if shallower and ref["mk_shallow"] is None:
        depth = max_depth or make_desc(scene, w, h, 0, "pt").config.max_depth
        r = hippt.PythonRenderer(make_desc(scene, w, h, depth - 1, "pt"), device_id=0)
        r.renderer.render(spp)
        ref["mk_shallow"] = r.renderer.accum.cpu().numpy().copy()
        r.release()
    for s in seeds:
        if s not in ref["mk"]:
            r = hippt.PythonRenderer(make_desc(scene, w, h, max_depth, "pt"),
                                     device_id=0, seed_offset=s)
            r.renderer.render(spp)
            ref["mk"][s] = r.renderer.accum.cpu().numpy().copy()
            r.release()
    if cpu and ref["cpu"] is None:
        r = hippt.PythonRenderer(make_desc(scene, w, h, max_depth, "pt"), device_id=-1)
        r.renderer.render(spp)
        ref["cpu"] = r.renderer.accum.copy()
    return ref


def agreement(a, b, spp):
    """(relative difference of the means, share of values more than 25 % off)
    — the project's figures for 'same streams, different compile'."""
    a, b = a[..., :3] / spp, b[..., :3] / spp
    rel_mean = abs(a.mean() - b.mean()) / b.mean()
    off = (np.abs(a - b) / (b + 0.05) > 0.25).mean()
    return float(rel_mean), float(off)


# (id, scene, w, h, spp, max_depth (0 = the scene's own), env)
FUSED = [
    ("span2", "cornell", 96, 96, 8, 5, {"HIPPT_WF_SPAN": "2"}),
    ("span1", "cornell", 96, 96, 8, 5, {"HIPPT_WF_SPAN": "1"}),
    ("span3_last_cnt1", "cornell", 96, 96, 8, 6, {"HIPPT_WF_SPAN": "3"}),
    ("span8_default", "cornell", 96, 96, 8, 12, {}),
    # the last step runs on live rays with do_trace=0 only when its span
    # reaches the end of the path from a sort before max_depth
    ("span3_last_notrace", "cornell", 96, 96, 8, 5, {"HIPPT_WF_SPAN": "3"}),
    ("span2_compact", "cornell", 96, 96, 8, 5,
     {"HIPPT_WF_SPAN": "2", "HIPPT_WF_SORT": "compact"}),
    ("span2_raygen", "cornell", 96, 96, 8, 5,
     {"HIPPT_WF_SPAN": "2", "HIPPT_WF_PRIMARY_FUSE": "0"}),
    ("kitchen_span2", "kitchen", 160, 90, 4, 0, {"HIPPT_WF_SPAN": "2"}),
    ("env_balls_span2", "env-balls", 96, 54, 8, 0, {"HIPPT_WF_SPAN": "2"}),
]


@pytest.mark.parametrize("cid,scene,w,h,spp,max_depth,env", FUSED,
                         ids=[c[0] for c in FUSED])
def test_fused_pipeline_matches_megakernel(tmp_path, cid, scene, w, h, spp, max_depth, env):
    """k_wf_primary / k_wf_raygen, k_wf_step and the gathered sorts run the
    megakernel's estimator sample for sample (same path_shade_hit / path_step,
    same Sampler streams), so the image agrees pixel by pixel within the
    project's bound for the same streams under another compilation: means
    within 2 %, fewer than 5 % of values more than 25 % off; the same against
    the CPU render.  Measured figures: the table in the module docstring."""
    depth = max_depth or make_desc(scene, w, h, 0, "wfpt").config.max_depth
    accum, lines = run_worker(tmp_path, scene, w, h, spp, max_depth, env)
    # 1. the pipeline really ran
    span = int(env.get("HIPPT_WF_SPAN", DEFAULT_SPAN))
    check_log(lines, expected_sorts(depth + 1, span,
                                    primary_fuse=env.get("HIPPT_WF_PRIMARY_FUSE") != "0"),
              w * h, depth)
    # 3. finite, and every pixel got exactly spp samples
    assert accum.shape == (h, w, 4) and np.isfinite(accum).all()
    assert (accum[..., 3] == spp).all()
    # 2. agreement with the megakernel and with the CPU render
    ref = references(scene, w, h, spp, max_depth, shallower=True)
    mk, cpu = ref["mk"][0], ref["cpu"]
    same = np.array_equal(accum, mk)
    rm, om = agreement(accum, mk, spp)
    rc, oc = agreement(accum, cpu, spp)
    ndiff = int((accum != mk).sum())
    print(f"{cid}: live {[n for _, n in lines]} vs megakernel: identical={same} "
          f"({ndiff} of {accum.size} values differ, max |diff| "
          f"{float(np.abs(accum - mk).max()):.3e}) rel {100 * rm:.2e}% off {100 * om:.2e}% "
          f"| vs cpu: rel {100 * rc:.2e}% off {100 * oc:.2e}%")
    assert rm < 0.02 and om < 0.05, (cid, "megakernel", rm, om)
    assert rc < 0.02 and oc < 0.05, (cid, "cpu", rc, oc)
    # No shade lost.  The late bounces carry too little light for the bound
    # above to see one go missing (dropping k_wf_step's extra_bounces loop
    # moves the span-2 mean by 1.2 %, the span-8 mean by 0.1 %).  But the
    # streams are shared, so an image that lost its last shade IS the
    # megakernel's image at max_depth - 1: the render must lie nearer to the
    # megakernel at max_depth than to the one a bounce shallower.  Measured
    # mean |difference| (at max_depth / at max_depth - 1): cornell depth 5
    # 7e-10 / 9.2e-3, depth 6 6e-10 / 4.7e-3, depth 12 8e-10 / 1.3e-4,
    # kitchen 3.8e-7 / 7.0e-3, env-balls 2.7e-9 / 1.9e-3; with the loop
    # dropped, span 2: 9.2e-3 / 5e-10, span 8: 7.5e-4 / 6.2e-4.
    d_full = float(np.abs(accum[..., :3] - mk[..., :3]).mean()) / spp
    d_shallow = float(np.abs(accum[..., :3] - ref["mk_shallow"][..., :3]).mean()) / spp
    print(f"{cid}: mean |wf - megakernel| {d_full:.3e} at max_depth, "
          f"{d_shallow:.3e} at max_depth - 1")
    assert d_full < d_shallow, (cid, d_full, d_shallow)


def block_means(accum, spp, bs=8):
    img = accum[..., :3] / spp
    h, w, _ = img.shape
    return img.reshape(h // bs, bs, w // bs, bs, 3).mean(axis=(1, 3))


def block_dist(a, b):
    return float((np.abs(a - b) / (b + 0.05)).max())


SPLIT = [("split", {}), ("split_dual", {"HIPPT_WF_DUAL": "1"})]


@pytest.mark.parametrize("cid,extra", SPLIT, ids=[c[0] for c in SPLIT])
def test_split_pipeline_matches_megakernel_statistically(tmp_path, cid, extra):
    """k_wf_shade / k_wf_shadow / k_wf_trace(_dual) are a separate
    implementation of the bounce, so nothing is assumed about the order of
    its random numbers: 8x8 block means of a 64 spp cornell box must lie
    within twice the largest seed-to-seed distance of four megakernel
    renders (D = max over blocks of |a-b|/(b+0.05); six pairs), and the image
    mean within twice their largest pairwise mean difference.  The factor 2:
    the maximum of six draws understates the tail for a seventh, while a
    lost NEE term or a dropped shadow queue moves block means by tens of
    percent."""
    scene, w, h, spp, depth = "cornell", 64, 64, 64, 5
    env = dict(extra, HIPPT_WF_FUSE="0", HIPPT_WF_SPAN="1")
    accum, lines = run_worker(tmp_path, scene, w, h, spp, depth, env)
    check_log(lines, expected_sorts(depth + 1, 1, fuse=False), w * h, depth)
    assert np.isfinite(accum).all() and (accum[..., 3] == spp).all()
    seeds = (0, 1, 2, 3)
    mk = references(scene, w, h, spp, depth, seeds=seeds, cpu=False)["mk"]
    bm = {s: block_means(mk[s], spp) for s in seeds}
    means = {s: float(mk[s][..., :3].mean() / spp) for s in seeds}
    pairs = [(a, b) for a in seeds for b in seeds if a < b]
    d_ref = max(block_dist(bm[a], bm[b]) for a, b in pairs)
    m_ref = max(abs(means[a] - means[b]) for a, b in pairs)
    d = block_dist(block_means(accum, spp), bm[0])
    m = abs(float(accum[..., :3].mean() / spp) - means[0])
    print(f"{cid}: identical to megakernel seed 0: {np.array_equal(accum, mk[0])}, "
          f"{int((accum != mk[0]).sum())} of {accum.size} values differ")
    print(f"{cid}: live {[n for _, n in lines]} D {d:.3e} (D_ref {d_ref:.4f}, bound "
          f"{2 * d_ref:.4f}) mean diff {m:.3e} (largest pairwise {m_ref:.5f}, "
          f"bound {2 * m_ref:.5f}, mean {means[0]:.4f})")
    assert d <= 2 * d_ref, (cid, d, d_ref)
    assert m <= 2 * m_ref, (cid, m, m_ref)


def test_wavefront_refuses_more_than_2_24_pixels():
    """Sort entries carry the pixel id in 24 bits: a 4097x4096 wfpt frame is
    refused with an error that names the limit, before anything is allocated
    or rendered (null buffers would fault otherwise)."""
    d = make_desc("cornell", 4097, 4096, 2, "wfpt")
    scene = hippt.Scene(d)
    scene.upload(0)
    with pytest.raises(RuntimeError, match=r"16777216 pixels \(2\^24"):
        scene.native.render_device(0, 0, 0, 1, 0, C.R_WAVEFRONT_PT, 0, 1.0, 0)
    scene.native.release()
