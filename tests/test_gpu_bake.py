"""Bake maps on the device (qa_bake_texels*, qa_bake_dilate_device: qa_bake.hip; the opening comment of qa_bake_dev.h is the
specification): the device build equals the host build bit for bit on every case of tests/test_bake_host.py that a context accepts -
at the tile edge, with one-lane waves, across the face-chunk boundary, on a resident scene and on one in global memory; the renderer's
own queries agree about the surface (a ray cast at a texel's point meets that point) and about the texel (the radiance of a ray at it is
the texel's colour, through the texmap); Context.bake_ao is the composition of its parts and leaves the scene an upload of the
downloaded blob would."""
import numpy as np
import pytest

import bake_util as B

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    root = tmp_path_factory.mktemp("gpu_bake")
    c = B.build_cases(root, uploadable=True)
    # 3200 faces: too large for the LDS-resident integrator, so the scene stays in global memory
    blob = B.write_scene(str(root / "big"), B.mesh_node("g.obj", '<rotate angle="30" z="1"/><translate z="1"/>'), {"g.obj": B.grid_obj(40, 40, height=B.dome)})
    c["big"] = {"blob": blob, "node": 1, "texmap": None, "mtl": -1, "sizes": ((33, 20),)}
    return c


@pytest.fixture(scope="module")
def ctx():
    from qaray_amd import hip
    c = hip.Context(0)
    yield c
    c.close()


def same_bits(x, y):
    from qaray_amd import hip
    return [k for k in hip.BAKE_PLANES if not np.array_equal(np.asarray(x[k]).view(np.uint32), np.asarray(y[k]).view(np.uint32))]


def device_map(ctx, c, size, **kw):
    out = ctx.bake_texels_device(c["node"], *size, texmap=c["texmap"], mtl=c["mtl"], **kw)
    ctx.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def test_device_equals_host_bit_for_bit(ctx, cases):
    import torch
    from qaray_amd import hip
    sizes = {s for c in cases.values() for s in c["sizes"]}
    assert {(1, 1), (16, 16), (17, 16), (19, 13)} <= sizes
    names = {}
    for name, c in cases.items():
        ctx.upload_scene(c["blob"])
        names[name] = ctx.kernel_name()
        for size in c["sizes"]:
            want = hip.bake_texels_host(c["blob"], c["node"], *size, texmap=c["texmap"], mtl=c["mtl"])
            got = device_map(ctx, c, size)
            assert not same_bits(got, want), (name, size, same_bits(got, want))
            if size == c["sizes"][0]:
                assert not same_bits(ctx.bake_texels(c["node"], *size, texmap=c["texmap"], mtl=c["mtl"]), want), (name, "host form")
                W, H = size
                only = device_map(ctx, c, size, face=torch.full((H, W), -5, dtype=torch.int32, device="cuda"))
                assert list(only) == ["face"] and np.array_equal(only["face"], want["face"])
    # the face-chunk boundary: some texel's winner lies in the second chunk of 256; three faces; both kinds of scene
    g = hip.bake_texels_host(cases["grid264"]["blob"], 1, 64, 64)["face"]
    assert len(B.mesh_arrays(cases["grid264"]["blob"], 0)["faces"]) == 264 and (g >= 256).any() and (g < 256).any()
    assert len(B.mesh_arrays(cases["tri3"]["blob"], 0)["faces"]) == 3
    print(f"chart: {names['chart']}; big: {names['big']}")
    assert "RES=1" in names["chart"] and "RES=1" not in names["big"]


def test_device_refusals_write_nothing(ctx, cases, tmp_path):
    import torch
    from qaray_amd import hip
    fresh = hip.Context(0)
    try:
        with pytest.raises(hip.HipError) as e:
            fresh.bake_texels(1, 4, 4)
        assert e.value.code == -5   # QA_ENOSCENE
    finally:
        fresh.close()
    five = B.write_scene(tmp_path / "five", B.mesh_node("s.obj"), {"s.obj": B.span_obj(5)})
    ctx.upload_scene(five)
    face = torch.full((4, 4), 77, dtype=torch.int32, device="cuda")
    with pytest.raises(hip.HipError) as e:
        ctx.bake_texels_device(1, 4, 4, face=face)
    ctx.synchronize()
    assert e.value.code == B.EUNSUPPORTED and (face.cpu().numpy() == 77).all()
    ctx.upload_scene(cases["chart"]["blob"])
    for node in (0, 2, -1):
        with pytest.raises(hip.HipError) as e:
            ctx.bake_texels_device(node, 4, 4, face=face)
        assert e.value.code == B.EINVAL, node
    for w, h in ((0, 4), (4, 0), (8193, 4), (4, 8193)):   # (the C entry itself: the binding would refuse the tensor's shape first)
        assert hip.lib().qa_bake_texels_device(ctx._h, 1, -1, -1, w, h, None, None, face.data_ptr(), None, None) == B.EINVAL, (w, h)
    with pytest.raises(hip.HipError) as e:
        ctx.bake_texels_device(1, 4, 4, texmap=0, face=face)
    assert e.value.code == B.EINVAL
    assert hip.lib().qa_bake_texels_device(ctx._h, 1, -1, -1, 4, 4, None, None, None, None, None) == B.EINVAL
    with pytest.raises(hip.HipError):
        ctx.bake_dilate_device(torch.zeros((4, 4, 3), dtype=torch.uint8, device="cuda"), face, 9)
    pic = torch.zeros((4, 4, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(hip.HipError) as e:
        ctx.bake_dilate_device(pic, face, 1, out=pic)
    assert e.value.code == B.EINVAL
    ctx.synchronize()
    assert (face.cpu().numpy() == 77).all()


def test_dilation_device_equals_host(ctx):
    import torch
    from qaray_amd import hip
    rng = np.random.default_rng(12)
    for (h, w), density in (((1, 1), 0.0), ((16, 16), 0.05), ((16, 17), 0.1), ((13, 19), 0.3), ((33, 40), 0.01), ((70, 50), 0.002)):
        rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        face = np.where(rng.random((h, w)) < density, 3, -1).astype(np.int32)
        for radius in (0, 1, 2, 8):
            got = ctx.bake_dilate_device(torch.from_numpy(rgb).cuda(), torch.from_numpy(face).cuda(), radius)
            ctx.synchronize()
            assert np.array_equal(got.cpu().numpy(), hip.bake_dilate_host(rgb, face, radius)), (h, w, radius)


def rays_at(m):
    """The rays at the covered texels of a device map: from 0.01 along the normal, against it -> (indices, origins, dirs)"""
    import torch
    idx = torch.nonzero(m["face"].reshape(-1) >= 0).reshape(-1)
    p, n = m["point"].reshape(-1, 3)[idx], m["normal"].reshape(-1, 3)[idx]
    return idx, (p + 0.01 * n).contiguous(), (-n).contiguous()


@pytest.mark.parametrize("name", ["convex", "plane_inset"])
def test_the_renderer_agrees_about_the_surface(ctx, cases, name):
    """cast_rays at every covered texel's point meets the node there: t within the point's own tolerance of 0.01, the hit within it of
    the map's point (tests/bake_util.py point_tolerance, as tests/test_bake_host.py derives it; nothing is added for the cast)."""
    c = cases[name]
    ctx.upload_scene(c["blob"])
    for size in c["sizes"]:
        m = ctx.bake_texels_device(c["node"], *size, texmap=c["texmap"])
        ctx.synchronize()   # (the map ran on the context's stream; torch reads it next)
        idx, o, d = rays_at(m)
        hit = ctx.cast_rays_device(o, d)
        ctx.synchronize()
        assert len(idx) > 100
        host = {k: v.cpu().numpy() for k, v in m.items()}
        _, _, scale = B.point_normal_f64(c["blob"], c["node"], host["face"], host["bary"])
        tol = B.point_tolerance(scale.reshape(-1)[idx.cpu().numpy()], B.chain_levels(c["blob"], c["node"]))
        t, ids, point = hit["t"].cpu().numpy(), hit["ids"].cpu().numpy(), hit["point"].cpu().numpy()
        assert (ids[:, 0] == c["node"]).all(), f"{name} {size}: {(ids[:, 0] != c['node']).sum()} rays of {len(idx)} meet another node or nothing"
        err_t = np.abs(t.astype(np.float64) - 0.01)
        err_p = np.abs(point.astype(np.float64) - m["point"].reshape(-1, 3)[idx].cpu().numpy()).max(axis=1)
        print(f"{name} {size}: {len(idx)} rays; t error / tolerance at most {(err_t / tol).max():.3f}, point error / tolerance at most {(err_p / tol).max():.3f}")
        assert (err_t <= tol).all() and (err_p <= tol).all()


def test_the_renderer_agrees_about_the_texel(ctx, cases):
    """The emission texture's texel (ix, iy) is (8 ix, 16 iy, 0): the radiance of a ray at a covered texel's point, looked up unfiltered
    through the emission's texmap (scale, quarter turn, translate), names the texel.  Pins the row flip, the sample convention and the
    direction of the texmap's transform to textureSample itself."""
    c = cases["texmap"]
    ctx.upload_scene(c["blob"])
    W, H = 32, 16
    m = ctx.bake_texels_device(c["node"], W, H, texmap=c["texmap"])
    ctx.synchronize()   # (the map ran on the context's stream; torch reads it next)
    idx, o, d = rays_at(m)
    rgb, t, _ = ctx.radiance_rays_device(o, d, spp=1, max_bounce=0)
    ctx.synchronize()
    idx, rgb = idx.cpu().numpy(), rgb.cpu().numpy().astype(np.float64)
    assert len(idx) >= 200 and (t.cpu().numpy() < 1.0).all()
    ix, iy = idx % W, idx // W
    gx, gy = np.round(rgb[:, 0] * 255 / 8).astype(int) % W, np.round(rgb[:, 1] * 255 / 16).astype(int) % H
    bad = (gx != ix) | (gy != iy)
    assert not bad.any(), f"{bad.sum()} of {len(idx)} texels: first (ix, iy) {ix[bad][:4]}, {iy[bad][:4]} seen as {gx[bad][:4]}, {gy[bad][:4]}"
    assert np.abs(rgb[:, 2]).max() == 0.0
    # the raw uv is another map: the texmap matters
    raw = ctx.bake_texels_device(c["node"], W, H)
    ctx.synchronize()
    assert not np.array_equal(raw["face"].cpu().numpy(), m["face"].cpu().numpy())


LIGHTMAP = ('<material type="blinn" name="lm"><diffuse r="1" g="1" b="1" texture="lm.ppm"/><specular value="0.1"/><glossiness value="10"/></material>'
            '<material type="blinn" name="c"><diffuse r="1" g="1" b="1" texture="checkerboard"><color1 r="0.2" g="0.2" b="0.2"/><color2 r="0.8" g="0.8" b="0.8"/>'
            '</diffuse></material>')


def test_bake_ao_is_its_composition(ctx, tmp_path):
    import torch
    from qaray_amd import hip
    W, H, K = 24, 20, 16
    texels = np.random.default_rng(3).integers(0, 256, (H, W, 3), dtype=np.uint8)
    objects = ('<object type="plane" name="floor" material="c"><scale value="8"/></object>'
               '<object type="sphere" name="ball" material="m"><scale value="0.8"/><translate x="0.3" y="0.2" z="2.6"/></object>'
               + B.mesh_node("g.obj", '<rotate angle="30" z="1"/><translate z="0.2"/>', material="lm"))
    blob = B.write_scene(tmp_path / "ao", objects, {"g.obj": B.grid_obj(5, 4, seed=9, u0=0.2, u1=0.8, v0=0.25, v1=0.75, height=B.dome),
                                                   "lm.ppm": B.ppm_bytes(texels)}, extra=B.MATTE + LIGHTMAP + B.LAMP)
    node = 3
    mats = hip.blob_table(blob, "materials")
    texmap = int(mats[[i for i in range(len(mats)) if mats[i]["diffuse"]["texmap"] >= 0 and
                       hip.blob_table(blob, "textures")[hip.blob_table(blob, "texmaps")[mats[i]["diffuse"]["texmap"]]["texture"]]["type"] == hip.QA_TEX_FILE][0]]["diffuse"]["texmap"])
    tex = int(hip.blob_table(blob, "texmaps")[texmap]["texture"])
    assert np.array_equal(hip.blob_texels(blob, tex), texels)
    ctx.upload_scene(blob)
    out = ctx.bake_ao(node, texmap, K=K, dilate=2)
    torch.cuda.synchronize()
    ctx.synchronize()
    # the parts, called one by one
    m = ctx.bake_texels_device(node, W, H, texmap=texmap)
    ids = torch.arange(W * H, dtype=torch.int32, device="cuda")
    ao = ctx.ao_points_device(m["point"].reshape(-1, 3), m["normal"].reshape(-1, 3), K, stream_ids=ids)["ao"].reshape(H, W)
    grey = ctx.ao_grey_device(out["ao"])
    ctx.synchronize()
    face = m["face"].cpu().numpy()
    cov = face >= 0
    assert np.array_equal(out["face"].cpu().numpy(), face) and 60 < cov.sum() < W * H - 60
    assert np.array_equal(out["ao"].cpu().numpy().view(np.uint32)[cov], ao.cpu().numpy().view(np.uint32)[cov])
    got_ao = out["ao"].cpu().numpy()
    assert got_ao[cov].min() < 0.9 and got_ao[cov].max() > 0.9, "the ball shades part of the cap"
    rgb8 = out["rgb8"].cpu().numpy()
    g = grey.cpu().numpy()
    assert (rgb8[cov] == g[cov][:, None]).all()
    before = np.where(cov[..., None], np.repeat(g[..., None], 3, axis=2), texels)
    assert np.array_equal(rgb8, B.dilate_ref(before, face, 2))
    # (of the uncovered texels some lie within two texels of the chart and are filled, the others keep the texture's bytes)
    assert (rgb8[~cov] == texels[~cov]).all(axis=1).any() and (rgb8[~cov] != texels[~cov]).any(axis=1).any()
    # the scene holds the bytes, and renders as an upload of the downloaded blob does
    down = ctx.download_scene()
    assert np.array_equal(hip.blob_texels(down, tex), rgb8)
    frame = ctx.render_region((0, 0, 48, 36), 2)
    other = hip.Context(0)
    try:
        other.upload_scene(down)
        again = other.render_region((0, 0, 48, 36), 2)
    finally:
        other.close()
    for x, y in zip(frame[:3], again[:3]):
        assert np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32))
    # a texmap whose texture is a checker has no texels to bake into
    checker = int(mats[[i for i in range(len(mats)) if mats[i]["diffuse"]["texmap"] >= 0 and int(mats[i]["diffuse"]["texmap"]) != texmap][0]]["diffuse"]["texmap"])
    with pytest.raises(hip.HipError) as e:
        ctx.bake_ao(node, checker)
    assert e.value.code == B.EINVAL
