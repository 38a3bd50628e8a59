"""What the radiance-query tests share (qa_radiance.hip: qa_radiance_rays*, qa_camera_sample_rays_device): the scene list of the
frame-parity anchor, and the frame / batch pair that anchor compares.  Frames, region and seeds are gbuffer_util's."""
import os
import re

import numpy as np

from conftest import GOLDEN, ROOT, reference_input_names
from gbuffer_util import REGION, scene_blob
from ray_query_util import H, W, with_camera

QA_EINVAL, QA_ENOSCENE, QA_EUNSUPPORTED = -1, -5, -6
SOFTSHADOW = "custom_softshadow.xml"
SOFTSHADOW_PINHOLE = dict(pos=(0, -30, 12), target=(0, 0, 3), up=(0, 0, 1), dof=0.0)   # the scene's own camera without its lens
TEXEDGE_SMALL = os.path.join(GOLDEN, "texedge", "texedge_small.xml")
TEXEDGE_BIG = os.path.join(GOLDEN, "texedge", "texedge_big.xml")
N = H * W


def xml_dof(name):
    """The <dof value=...> of a scene file's camera (0 when it has none): what decides at collection time, without loading the
    scene, whether a reference input belongs to the anchor; the anchor asserts it against the blob's camera record"""
    text = open(os.path.join(ROOT, "scenes", name)).read()
    m = re.search(r"<dof\s+value\s*=\s*\"([^\"]+)\"", text)
    return float(m.group(1)) if m else 0.0


PINHOLE_INPUTS = [n for n in reference_input_names() if xml_dof(n) <= 0.1]
LENS_INPUTS = [n for n in reference_input_names() if xml_dof(n) > 0.1]
# no committed scene file has area lights, no texture and meshes in global memory at once: example_project11_box.xml with its point
# light given a size reaches that instance, <RES=0,LIGHTS=1,TEX=0,AREA=1>
AREA_BOX = "example_project11_box.xml with an area light"
QA_LIGHT_POINT = 2
ANCHOR_SCENES = PINHOLE_INPUTS + [SOFTSHADOW, TEXEDGE_SMALL, TEXEDGE_BIG, "custom_textures.xml", AREA_BOX]
ORACLE_SCENES = ("example_project12_box.xml", "example_project3_sphere.xml", TEXEDGE_BIG)


def anchor_blob(scene):
    if scene == AREA_BOX:
        from qaray_amd import hip
        blob = scene_blob("example_project11_box.xml").copy()
        lights = hip.blob_table(blob, "lights")
        assert (lights["type"] == QA_LIGHT_POINT).sum() == 1
        lights["size"][lights["type"] == QA_LIGHT_POINT] = 1.5
        return blob
    blob = scene_blob(scene)
    if scene == SOFTSHADOW:
        blob = with_camera(scene, blob, **SOFTSHADOW_PINHOLE)
    return blob


def variant(kernel_name):
    """(RES, LIGHTS, TEX, AREA) of a kernel_name() with cooperative walks off"""
    return tuple(int(f"{k}=1" in kernel_name) for k in ("RES", "LIGHTS", "TEX", "AREA"))


def frame(c, spp, seed, max_bounce=5):
    """render_region_device of REGION -> (rgb [N,3], depth [N], ns [N]) numpy, and the counters of that frame alone"""
    import torch
    rgb = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")
    depth = torch.zeros((H, W), dtype=torch.float32, device="cuda:0")
    ns = torch.zeros((H, W), dtype=torch.int32, device="cuda:0")
    c.reset_counters()
    c.render_region_device(REGION, spp, rgb, depth, ns, max_bounce=max_bounce, seed=seed)
    c.synchronize()
    return (rgb.cpu().numpy().reshape(N, 3), depth.cpu().numpy().reshape(N), ns.cpu().numpy().reshape(N)), c.counters()


def batch_of_own_rays(c, spp, seed, max_bounce=5, **drop):
    """radiance_rays_device(camera_sample_rays_device(REGION, 0, spp, all outputs), per sample) -> (rgb, t, ns) numpy, the counters
    of that batch alone, and the rays (tensors).  drop: names of camera_sample outputs to leave out of the call (dx=True, ...)"""
    rays = c.camera_sample_rays_device(REGION, 0, spp)
    kw = dict(dx=rays["dx"], dy=rays["dy"], screen=rays["screen"], stream_ids=rays["stream_ids"])
    for k in drop:
        kw[k] = None
    c.reset_counters()
    out = c.radiance_rays_device(rays["origins"], rays["dirs"], spp=spp, max_bounce=max_bounce, seed=seed, **kw)
    c.synchronize()
    return tuple(a.cpu().numpy() for a in out), c.counters(), rays
