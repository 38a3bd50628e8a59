"""Context.bake_light(photon_maps=True) on the 32 x 32 fixture of tests/golden/bake_light with its ball made of refractive glass (the
record of custom_photon.xml's `glass`): the light map is the composition tests/test_gpu_bake_light.py writes out, with the flag on
its point query, so the chart under the ball holds the caustic a frame with maps shows; the texel edit at its end drops the maps.
tests/test_radiance_photon_oracle.py checks on the CPU that the map sizes fill."""
import os

import numpy as np
import pytest

import bake_util as B
from radiance_util import variant
from test_gpu_bake_light import FIXTURE, H, NODE, W, lightmap_of

pytestmark = pytest.mark.gpu

PHOTON, CAUSTICS = (2000, 20, 0.5), (200, 20, 1.0)
BALL_DIFFUSE = (0.7, 0.6, 0.5)


def glass_ball_blob():
    """The fixture's blob with the ball's material record replaced by custom_photon.xml's glass"""
    from qaray_amd import hip
    from qaray_amd.host import load_scene_blob
    blob = load_scene_blob(os.path.join(FIXTURE, "scene.xml"), size=(48, 36), asset_root=FIXTURE).copy()
    donor = hip.blob_table(load_scene_blob("custom_photon.xml", size=(48, 36)), "materials")
    glass = [m for m in donor if np.allclose(m["refraction"]["color"], 0.95) and float(m["ior"]) == 1.5]
    assert len(glass) == 1 and all(int(glass[0][f]["texmap"]) < 0 for f in ("diffuse", "specular", "reflection", "refraction", "emission"))
    mats = hip.blob_table(blob, "materials")
    ball = [i for i, m in enumerate(mats) if np.allclose(m["diffuse"]["color"], BALL_DIFFUSE)]
    assert len(ball) == 1
    mats[ball[0]] = glass[0]
    return blob


def test_bake_light_with_maps_is_its_composition_with_the_flag():
    import torch
    from qaray_amd import hip
    blob = glass_ball_blob()
    texmap, tex = lightmap_of(blob)
    texels = hip.blob_texels(blob, tex).copy()
    spp, bounces, scale = 8, 2, 0.5
    ctx, other = hip.Context(0), hip.Context(0)
    try:
        for c in (ctx, other):
            c.set_option("coop", 0)
            c.upload_scene(blob.copy())
            c.build_photon_maps(PHOTON, CAUSTICS)
        inst = variant(ctx.kernel_name())
        print("instance <RES, LIGHTS, TEX, AREA>:", inst)
        assert inst == (1, 1, 1, 0), "qa_integrate_points_pm<RES=1, TEX=1, AREA=0>"
        out = ctx.bake_light(NODE, texmap, spp=spp, max_bounce=bounces, scale=scale, dilate=2, photon_maps=True)
        torch.cuda.synchronize()
        ctx.synchronize()
        assert sorted(out) == ["face", "light", "rgb8"] and tuple(out["light"].shape) == (H, W, 3)
        with pytest.raises(hip.HipError, match="no photon maps"):   # the texel edit dropped them: the caller rebuilds
            ctx.photon_maps_info()
        down = ctx.download_scene()
        # the parts, called one by one on a context that holds the scene as it was, maps built
        m = other.bake_texels_device(NODE, W, H, texmap=texmap)
        ids = torch.arange(W * H, dtype=torch.int32, device="cuda")
        pts, nrm = m["point"].reshape(-1, 3), m["normal"].reshape(-1, 3)
        light = other.irradiance_points_device(pts, nrm, spp, bounces, stream_ids=ids, photon_maps=True)[0].reshape(H, W, 3)
        other.synchronize()   # (torch's product below is not ordered behind the context's stream)
        grey = other.ao_grey_device(light * scale)
        other.synchronize()
        face = m["face"].cpu().numpy()
        cov = face >= 0
        assert np.array_equal(out["face"].cpu().numpy(), face) and 60 < cov.sum() < W * H - 60
        got = out["light"].cpu().numpy()
        assert np.array_equal(got.view(np.uint32), light.cpu().numpy().view(np.uint32))
        assert not got[~cov].any(), "an uncovered texel is a void point"
        before = np.where(cov[..., None], grey.cpu().numpy(), texels)
        want = B.dilate_ref(before, face, 2)
        rgb8 = out["rgb8"].cpu().numpy()
        assert np.array_equal(rgb8, want)
        assert np.array_equal(hip.blob_texels(down, tex), rgb8), "the scene holds the bytes"
        # the maps arrive in the map: without them the light at some covered texels is another
        other.clear_photon_maps()
        plain = other.irradiance_points_device(pts, nrm, spp, bounces, stream_ids=ids)[0].reshape(H, W, 3)
        other.synchronize()
        differ = (plain.cpu().numpy().view(np.uint32) != got.view(np.uint32)).any(axis=2)
        print("covered texels whose light the maps change:", int(differ[cov].sum()), "of", int(cov.sum()))
        assert differ[cov].any() and not differ[~cov].any()
    finally:
        ctx.close()
        other.close()
