"""Child process of tests/test_gpu_visit.py: render one small scene with a
megakernel renderer and save the accumulation buffer.  launch_render reads
HIPPT_OCC once per process, so every value needs a process of its own; the
parent sets the environment.

usage: occ_worker.py RENDERER SPP OUT.npy      (RENDERER: pt | vpt)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WIDTH, HEIGHT = 64, 36


def make_desc(renderer):
    from hippt.scene.procedural import kitchen, smoke_box
    if renderer == "pt":
        return kitchen(width=WIDTH, height=HEIGHT, detail=0.25, renderer="pt")
    if renderer == "vpt":
        return smoke_box(width=WIDTH, height=HEIGHT, n_grid=32, renderer="vpt")
    raise ValueError(renderer)


def main(argv):
    renderer, spp, out = argv
    import numpy as np
    import hippt
    r = hippt.PythonRenderer(make_desc(renderer), device_id=0)
    r.renderer.render(int(spp))
    np.save(out, r.renderer.accum.cpu().numpy())
    r.release()
    sys.stdout.flush()


if __name__ == "__main__":
    main(sys.argv[1:])
