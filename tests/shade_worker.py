"""Child process of tests/test_gpu_shade_render.py: render one named scene on
the GPU and save the image, so that every render has a time limit of its own.

usage: shade_worker.py SCENE RENDERER WIDTH HEIGHT SPP OUT.npy
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

XML_SCENES = ("balls", "spot-cbox", "point-cbox", "env-balls")


def make_desc(scene, renderer, width, height):
    if scene in XML_SCENES:
        from hippt.scene.xml_parser import parse_xml
        d = parse_xml(os.path.join(ROOT, "scenes", scene + ".xml"))
        d.camera.width, d.camera.height = width, height
        d.config.renderer = renderer
        return d
    if scene == "spheres":
        import shade_util as su
        return su.spheres_scene(width=width, height=height, renderer=renderer)
    raise ValueError(scene)


def main(argv):
    scene, renderer, width, height, spp, out = argv
    import numpy as np
    import hippt
    d = make_desc(scene, renderer, int(width), int(height))
    r = hippt.PythonRenderer(d, device_id=0)
    img = r.render(spp=int(spp)).cpu().numpy()
    np.save(out, img)
    r.release()
    sys.stdout.flush()


if __name__ == "__main__":
    main(sys.argv[1:])
