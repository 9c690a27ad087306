"""Child process of tests/test_gpu_wavefront.py: render one named scene with
renderer="wfpt" and save the accumulation buffer.  The wavefront launcher
reads its HIPPT_WF_* hooks once per process, so every configuration needs a
process of its own; the parent sets the environment.

usage: wf_worker.py SCENE WIDTH HEIGHT SPP MAX_DEPTH OUT.npy
       (MAX_DEPTH 0 keeps the scene's own)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_desc(scene, width, height, max_depth, renderer):
    """The scenes of the wavefront pipeline tests, by name."""
    from hippt.scene.procedural import cornell_box, kitchen
    if scene == "cornell":
        # cornell_box derives the per-lobe caps from max_depth
        return cornell_box(width=width, height=height, renderer=renderer,
                           **({"max_depth": max_depth} if max_depth > 0 else {}))
    elif scene == "kitchen":
        d = kitchen(width=width, height=height, renderer=renderer)
    elif scene == "env-balls":
        from hippt.scene.xml_parser import parse_xml
        d = parse_xml(os.path.join(ROOT, "scenes", "env-balls.xml"))
        d.camera.width, d.camera.height = width, height
        d.config.renderer = renderer
    else:
        raise ValueError(scene)
    if max_depth > 0:
        d.config.max_depth = max_depth
    return d


def main(argv):
    scene, width, height, spp, max_depth, out = argv
    import numpy as np
    import hippt
    d = make_desc(scene, int(width), int(height), int(max_depth), "wfpt")
    r = hippt.PythonRenderer(d, device_id=0)
    r.renderer.render(int(spp))
    np.save(out, r.renderer.accum.cpu().numpy())
    r.release()
    sys.stdout.flush()


if __name__ == "__main__":
    main(sys.argv[1:])
