"""The batch driver's -ao [K] and -ao-radius R: <prefix>aoBuffer.png is the 8-bit grey picture of the ambient occlusion of the frame's
own samples, made on the GPU; the three standard images stay byte for byte; -devices and a lens camera are refused before rendering."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from matte_util import linear_byte

pytestmark = pytest.mark.gpu
BOX, DOF_SCENE = "example_project12_box.xml", "custom_softshadow.xml"
SIZE = (48, 36)
NAMES = ("colorBuffer.png", "depthBuffer.png", "sampleBuffer.png")


def test_cli_ao_writes_the_occlusion_and_leaves_the_three(tmp_path):
    from PIL import Image
    from qaray_amd import hip
    from qaray_amd.host import SCENES_DIR, load_scene_blob
    exe = os.path.join(ROOT, "qaray_amd", "lib", "qaray_hip")
    common = ["-batch", "-spp", "4", "-bounce", "5", "-size", str(SIZE[0]), str(SIZE[1]), "-root", SCENES_DIR]
    run = lambda args: subprocess.run([exe] + common + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)   # noqa: E731
    modes = {"plain": [], "ao": ["-ao"], "ao8": ["-ao", "8", "-ao-radius", "6.5"], "prog": ["-ao", "8", "-ao-radius", "6.5", "-progressive", "2"]}
    outs = {}
    for mode, extra in modes.items():
        outs[mode] = str(tmp_path / mode) + "_"
        r = run(extra + ["-out", outs[mode], os.path.join(SCENES_DIR, BOX)])
        assert r.returncode == 0, r.stdout
    assert not os.path.exists(outs["plain"] + "aoBuffer.png")
    for mode in ("ao", "ao8", "prog"):
        for png in NAMES:
            with open(outs["plain"] + png, "rb") as a, open(outs[mode] + png, "rb") as b:
                assert a.read() == b.read(), (mode, png)
    c = hip.Context(0)
    try:
        c.upload_scene(load_scene_blob(BOX, size=SIZE))
        region = (0, 0) + SIZE
        for mode, (k, radius) in {"ao": (4, float("inf")), "ao8": (8, 6.5)}.items():
            img = Image.open(outs[mode] + "aoBuffer.png")
            assert img.mode == "L" and img.size == SIZE
            grey = np.asarray(img)
            planes = c.ao_device(region, 4, k, radius)      # (-spp 4: every pixel of the frame holds four samples)
            dev_grey = c.ao_grey_device(planes["ao"])
            c.synchronize()
            want = linear_byte(planes["ao"].cpu().numpy())
            assert np.array_equal(dev_grey.cpu().numpy(), want)
            assert np.array_equal(grey, want), mode
            print(mode, "grey levels:", len(np.unique(grey)), "min", grey.min(), "max", grey.max())
            assert len(np.unique(grey)) > 4
    finally:
        c.close()
    with open(outs["ao8"] + "aoBuffer.png", "rb") as a, open(outs["prog"] + "aoBuffer.png", "rb") as b:
        assert a.read() == b.read()      # the last pass of the progressive frame holds the same samples
    r = run(["-ao", "-devices", "2", os.path.join(SCENES_DIR, BOX)])
    assert r.returncode != 0 and "-ao" in r.stdout and "-devices" in r.stdout
    r = run(["-ao", "-out", str(tmp_path / "lens") + "_", os.path.join(SCENES_DIR, DOF_SCENE)])
    assert r.returncode != 0 and "-ao" in r.stdout and "pinhole" in r.stdout and not os.path.exists(str(tmp_path / "lens") + "_colorBuffer.png")
    r = run(["-ao", "300", os.path.join(SCENES_DIR, BOX)])
    assert r.returncode != 0 and "-ao" in r.stdout
