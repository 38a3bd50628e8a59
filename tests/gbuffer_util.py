"""What the G-buffer tests share: the scenes (one per <RES, TEX> instantiation of qa_gbuffer), the odd region, and the
"emission := diffuse" twin of a scene whose oracle frame at one sample and no bounce IS the albedo plane on hit pixels."""
import os

import numpy as np

from conftest import GOLDEN, ensure_assets

MISS = np.float32(1.0e30)
SIZE = (64, 48)
REGION = (5, 3, 52, 43)   # origin not (0, 0), 47 x 40 pixels: neither a multiple of 8, 6 x 5 tiles
SEEDS = (0x51A7A7, 12345)
# scene -> the instantiation it reaches (asserted against kernel_name() with cooperative walks off)
SCENES = {
    "example_project12_box.xml": (1, 0),                                   # <RES, !TEX>: the LDS-resident Cornell box
    os.path.join(GOLDEN, "texedge", "texedge_small.xml"): (1, 1),          # <RES, TEX>
    "example_project11_teapot.xml": (0, 0),                                # <!RES, !TEX>: the teapot in global memory
    os.path.join(GOLDEN, "texedge", "texedge_big.xml"): (0, 1),            # <!RES, TEX>
    "custom_textures.xml": None,                                           # textured; whichever memory it lands in
}


def scene_blob(scene, size=SIZE):
    from qaray_amd.host import load_scene_blob
    ensure_assets()
    return load_scene_blob(scene, size=size)


def emission_twin(blob):
    """A copy of the blob in which every material emits its diffuse texcolor and does nothing else."""
    from qaray_amd import hip
    twin = blob.copy()
    m = hip.blob_table(twin, "materials")
    m["emission"] = m["diffuse"]
    for k in ("diffuse", "specular", "reflection", "refraction"):
        m[k]["color"] = 0
    return twin


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)
