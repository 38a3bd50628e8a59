"""The construction tests/test_gpu_gbuffer.py checks the albedo plane with, established on the CPU: in the "emission := diffuse"
twin of an untextured scene (gbuffer_util.emission_twin) the oracle's frame at one sample and no bounce holds, at every hit pixel,
the diffuse colour of one of the scene's materials, bit for bit (a first hit returns 0 + 1 * emission, and the running mean of one
sample is that value).  No material class had to be excluded: the share of hit pixels left out is 0, and asserted."""
import numpy as np

from gbuffer_util import MISS, REGION, bits, emission_twin, scene_blob


def test_twin_frame_is_the_diffuse_colour_at_every_hit_pixel():
    from oracle import binding as oracle
    from qaray_amd import hip
    blob = scene_blob("example_project12_box.xml")
    rgb, depth, ns, _ = oracle.render(emission_twin(blob), REGION, 1, max_bounce=0)
    hit = depth != MISS
    assert hit.sum() > 500 and (ns == 1).all()
    diffuse = bits(np.ascontiguousarray(hip.blob_table(blob, "materials")["diffuse"]["color"]))
    px = bits(rgb.astype(np.float32))[hit]
    known = (px[:, None, :] == diffuse[None, :, :]).all(axis=2).any(axis=1)
    excluded = 1.0 - known.mean()
    print(f"hit pixels {hit.sum()}, distinct colours {len(np.unique(px, axis=0))}, excluded share {excluded:.4f}")
    assert excluded == 0.0
    assert len(np.unique(px, axis=0)) >= 2   # (more than one material is in view: the frame is not one constant)


def test_twin_keeps_geometry_and_texmaps():
    from qaray_amd import hip
    blob = scene_blob("custom_textures.xml")
    twin = emission_twin(blob)
    a, b = hip.blob_table(blob, "materials"), hip.blob_table(twin, "materials")
    assert np.array_equal(b["emission"]["texmap"], a["diffuse"]["texmap"]) and np.array_equal(bits(b["emission"]["color"]), bits(a["diffuse"]["color"]))
    assert not b["diffuse"]["color"].any() and not b["specular"]["color"].any()
    assert np.array_equal(hip.blob_table(blob, "instances"), hip.blob_table(twin, "instances"))
