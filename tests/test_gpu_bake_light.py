"""Context.bake_light (qaray_amd/hip.py) on the 32 x 32 fixture of tests/golden/bake_light: a domed chart that owns the file texture
lm.ppm, under a ball, over a checkered floor, lit by one point light.  The light map is the composition of the public calls it
names - bake_texels_device, irradiance_points_device, ao_grey_device, bake_dilate_device, edit_texels - and the scene holds its bytes
afterwards."""
import os

import numpy as np
import pytest

import bake_util as B
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, "bake_light")
W = H = 32
NODE = 3   # floor, ball, chart behind the root


@pytest.fixture(scope="module")
def blob():
    from qaray_amd.host import load_scene_blob
    return load_scene_blob(os.path.join(FIXTURE, "scene.xml"), size=(48, 36), asset_root=FIXTURE)


@pytest.fixture()
def ctx(blob):
    from qaray_amd import hip
    c = hip.Context(0)
    c.upload_scene(blob.copy())
    yield c
    c.close()


def lightmap_of(blob):
    """-> (texmap, texture) of the chart's file texture"""
    from qaray_amd import hip
    maps, textures = hip.blob_table(blob, "texmaps"), hip.blob_table(blob, "textures")
    texmap = [i for i in range(len(maps)) if int(textures[int(maps[i]["texture"])]["type"]) == hip.QA_TEX_FILE]
    assert len(texmap) == 1
    tex = int(maps[texmap[0]]["texture"])
    assert (int(textures[tex]["width"]), int(textures[tex]["height"])) == (W, H)
    return texmap[0], tex


def test_bake_light_is_its_composition(ctx, blob):
    import torch
    from qaray_amd import hip
    texmap, tex = lightmap_of(blob)
    texels = hip.blob_texels(blob, tex).copy()
    spp, bounces, scale = 8, 2, 0.5
    out = ctx.bake_light(NODE, texmap, spp=spp, max_bounce=bounces, scale=scale, dilate=2)
    torch.cuda.synchronize()
    ctx.synchronize()
    assert sorted(out) == ["face", "light", "rgb8"] and tuple(out["light"].shape) == (H, W, 3)
    down = ctx.download_scene()
    # the parts, called one by one on a context that holds the scene as it was
    other = hip.Context(0)
    try:
        other.upload_scene(blob.copy())
        m = other.bake_texels_device(NODE, W, H, texmap=texmap)
        ids = torch.arange(W * H, dtype=torch.int32, device="cuda")
        light = other.irradiance_points_device(m["point"].reshape(-1, 3), m["normal"].reshape(-1, 3), spp, bounces, stream_ids=ids)[0].reshape(H, W, 3)
        other.synchronize()   # (torch's product below is not ordered behind the context's stream)
        grey = other.ao_grey_device(light * scale)
        other.synchronize()
        face = m["face"].cpu().numpy()
        cov = face >= 0
        assert np.array_equal(out["face"].cpu().numpy(), face) and 60 < cov.sum() < W * H - 60
        got = out["light"].cpu().numpy()
        assert np.array_equal(got.view(np.uint32), light.cpu().numpy().view(np.uint32))
        assert not got[~cov].any(), "an uncovered texel is a void point"
        assert (got[cov] > 0).any() and len(np.unique(got[cov], axis=0)) > 60, "the lamp lights the cap, unevenly"
        g = grey.cpu().numpy()
        # linear bytes: the texel table decodes a byte by / 255, so the texture shows light * scale to half a step
        shown = hip.texels_host(g)[..., :3]
        inside = cov & (got * scale <= 1).all(axis=2)
        assert inside.sum() > 60 and np.abs(shown[inside] - got[inside] * scale).max() <= 0.5 / 255 + 1e-6
        before = np.where(cov[..., None], g, texels)
        want = B.dilate_ref(before, face, 2)
        rgb8 = out["rgb8"].cpu().numpy()
        assert np.array_equal(rgb8, want)
        filled = other.bake_dilate_device(torch.from_numpy(before).to("cuda"), m["face"], 2)
        other.synchronize()
        assert np.array_equal(rgb8, filled.cpu().numpy())
    finally:
        other.close()
    # uncovered texels out of reach of the fill keep their bytes; some within two texels of the chart are filled
    assert (rgb8[~cov] == texels[~cov]).all(axis=1).any() and (rgb8[~cov] != texels[~cov]).any(axis=1).any()
    reach = np.zeros_like(cov)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            reach |= np.roll(cov, (dy, dx), axis=(0, 1))   # (the fill wraps at the borders, as the texture lookup does)
    far = ~cov & ~reach
    assert far.sum() > 60 and np.array_equal(rgb8[far], texels[far])
    # the scene holds the bytes
    assert np.array_equal(hip.blob_texels(down, tex), rgb8)


def test_a_texmap_without_a_file_texture_is_refused(ctx, blob):
    from qaray_amd import hip
    texmap, _ = lightmap_of(blob)
    checker = [i for i in range(len(hip.blob_table(blob, "texmaps"))) if i != texmap][0]
    with pytest.raises(hip.HipError) as e:
        ctx.bake_light(NODE, checker)
    assert e.value.code == B.EINVAL
    with pytest.raises(hip.HipError):
        ctx.bake_light(NODE, 99)
