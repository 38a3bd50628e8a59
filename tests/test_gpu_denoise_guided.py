"""The guided filter on the device (qa_denoise_guided_device, qa_progressive_denoise_guided*: qa_denoise.hip): the device build of
the GUIDED FORM of qa_denoise_dev.h equals the host build (qa_test_denoise_guided_host, pinned to a restatement of the specification
by tests/test_denoise_guided_host.py) bit for bit, on plain frames and on progressive frames, whose guide planes the call computes
itself; the claim about quality on the renderer's own frames; the batch driver's -denoise-guided."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, ensure_assets
from denoise_guided_util import bits, guided_frame, luma

pytestmark = pytest.mark.gpu

QA_EINVAL = -1
BOX = "example_project12_box.xml"
TEXTURED = "custom_textures.xml"
# (w, h): smaller than a 16x16 tile; ragged in both dimensions; 40x33, where 6 iterations reach steps 1 - 32
SIZES = ((7, 5), (33, 17), (40, 33), (67, 45))


@pytest.fixture(scope="module")
def ctx():
    from qaray_amd import hip
    c = hip.Context(0)
    yield c
    c.close()


def blob(scene, size):
    from qaray_amd.host import load_scene_blob
    ensure_assets()
    return load_scene_blob(scene, size=size)


def upload(rgb, depth, ns, normal, albedo):
    import torch
    dev = torch.device("cuda", 0)
    f = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    return f(rgb), f(depth), torch.from_numpy(np.ascontiguousarray(ns, np.uint32).view(np.int32)).to(dev), f(normal), f(albedo)


def device_guided(ctx, frame, iterations, stream=None, alias=False):
    import torch
    t = upload(*frame)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    out = ctx.denoise_guided_device(*t, out=t[0] if alias else None, iterations=iterations, stream=stream.cuda_stream if stream is not None else None)
    if stream is not None:
        stream.synchronize()
    else:
        ctx.synchronize()
    for k, (dev, host) in enumerate(zip(t, frame)):   # the inputs are not written
        if dev is not None and not (alias and k == 0):
            assert np.array_equal(dev.cpu().numpy().view(np.uint32), np.ascontiguousarray(host).view(np.uint32)), k
    return out.cpu().numpy()


@pytest.mark.parametrize("w,h", SIZES)
def test_device_equals_host_bit_for_bit(ctx, w, h):
    import torch
    from qaray_amd import hip
    rgb, depth, ns, normal, albedo = guided_frame(w, h, 100 * w + h)
    side = torch.cuda.Stream()
    for guides in ((normal, albedo), (normal, None), (None, albedo), (None, None)):
        for iterations in (0, 1, 2, 3, 6):
            want = bits(hip.denoise_guided_host(rgb, depth, ns, *guides, iterations=iterations))
            for stream, alias in ((None, False), (side, True)) if iterations != 3 else ((None, True), (side, False)):
                got = bits(device_guided(ctx, (rgb, depth, ns) + guides, iterations, stream, alias))
                bad = np.argwhere(got != want)
                assert bad.size == 0, (guides[0] is not None, guides[1] is not None, iterations, stream is not None, alias, len(bad), bad[:5])


def test_a_smaller_frame_after_a_larger_one_and_the_unguided_filter_between():
    from qaray_amd import hip
    c = hip.Context(0)   # (its own context: the working planes start at the first frame's size)
    try:
        small, large = guided_frame(16, 16, 1), guided_frame(67, 45, 2)
        first = device_guided(c, small, 5)
        assert np.array_equal(bits(device_guided(c, large, 5)), bits(hip.denoise_guided_host(*large)))
        assert np.array_equal(bits(device_guided(c, small[:3] + (None, None), 5)), bits(hip.denoise_host(*small[:3])))
        assert np.array_equal(bits(device_guided(c, small, 5)), bits(first))
        assert np.array_equal(bits(first), bits(hip.denoise_guided_host(*small)))
    finally:
        c.close()


def test_progressive_frames_compute_their_own_guides(ctx):
    """An odd region with an origin that is not (0, 0): 47 x 40 pixels of the textured scene."""
    import torch
    from qaray_amd import hip
    size, region = (64, 48), (5, 3, 52, 43)
    ctx.upload_scene(blob(TEXTURED, size))
    with ctx.progressive(region, 16) as prog:
        for s in (4, 8):
            prog.advance(s)
            frame = prog.read()
            g = prog.gbuffer_device()
            ctx.synchronize()
            normal, albedo = g["normal"].cpu().numpy(), g["albedo"].cpu().numpy()
            want = hip.denoise_guided_host(*frame, normal, albedo)
            assert np.array_equal(bits(prog.denoise_guided()), bits(want))
            out = prog.denoise_guided_device()
            ctx.synchronize()
            assert np.array_equal(bits(out.cpu().numpy()), bits(want))
            side = torch.cuda.Stream()
            out = prog.denoise_guided_device(iterations=2, flags=hip.QA_DENOISE_GUIDE_NORMAL, stream=side.cuda_stream)
            side.synchronize()
            assert np.array_equal(bits(out.cpu().numpy()), bits(hip.denoise_guided_host(*frame, normal, None, iterations=2)))
            assert np.array_equal(bits(prog.denoise_guided(flags=0)), bits(prog.denoise()))
            plain, unguided = prog.denoise_device(), prog.denoise_guided_device(flags=0)
            ctx.synchronize()
            assert np.array_equal(bits(unguided.cpu().numpy()), bits(plain.cpu().numpy()))
            assert np.array_equal(bits(prog.denoise_guided(iterations=0)), bits(frame[0]))
            assert all(np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)) for a, b in zip(prog.read(), frame))
        assert not np.array_equal(bits(want), bits(hip.denoise_host(*frame)))


@pytest.fixture(scope="module")
def quality(ctx):
    """scene -> luma RMSE to the 256-spp frame of the raw 4-spp frame, its unguided and its guided filtering (defaults), 64x64."""
    out = {}
    region = (0, 0, 64, 64)
    for scene in (TEXTURED, BOX):
        ctx.upload_scene(blob(scene, (64, 64)))
        rgb, depth, ns = ctx.render_region(region, 4)
        many = luma(ctx.render_region(region, 256)[0].astype(np.float64))
        g = ctx.gbuffer(region)
        t = upload(rgb, depth, ns, g["normal"], g["albedo"])
        guided = ctx.denoise_guided_device(*t)
        plain = ctx.denoise_device(*t[:3])
        ctx.synchronize()
        rmse = lambda x: float(np.sqrt(np.mean((luma(np.asarray(x, np.float64)) - many) ** 2)))
        out[scene] = (rmse(rgb), rmse(plain.cpu().numpy()), rmse(guided.cpu().numpy()))
        print(f"{scene}: luma RMSE raw {out[scene][0]:.4f} unguided {out[scene][1]:.4f} guided {out[scene][2]:.4f}")
    return out


def test_guides_help_on_the_textured_scene_and_cost_nothing_on_the_box(quality):
    """Luma RMSE of the 4-spp frame to the 256-spp frame at 64x64, raw / unguided / guided with the defaults (host build on the
    device's frames, one MI355X run): custom_textures.xml 0.0325 / 0.0320 / 0.0312, Cornell box 0.8470 / 0.5189 / 0.5205."""
    raw, plain, guided = quality[TEXTURED]
    assert guided < plain
    assert guided < raw
    raw, plain, guided = quality[BOX]
    assert guided <= plain * 1.02
    assert guided < raw


def test_invalid_arguments_are_refused(ctx):
    import ctypes as C
    from qaray_amd import hip
    frame = guided_frame(7, 5, 3)
    t = upload(*frame)
    for kw in ({"iterations": 7}, {"sigma_normal": 0.0}, {"sigma_normal": float("nan")}, {"sigma_color": -1.0}):
        with pytest.raises(hip.HipError) as e:
            ctx.denoise_guided_device(*t, **kw)
        assert e.value.code == QA_EINVAL, kw
    L, ok = hip.lib(), hip.DenoiseGuidedParams.default()
    ptr = [x.data_ptr() for x in t]
    assert L.qa_denoise_guided_device(ctx._h, ptr[0], ptr[1], ptr[2], None, ptr[4], 7, 5, C.byref(ok), ptr[0], None) == QA_EINVAL   # bit without plane
    ok.flags = 2
    assert L.qa_denoise_guided_device(ctx._h, ptr[0], ptr[1], ptr[2], ptr[3], ptr[4], 7, 5, C.byref(ok), ptr[0], None) == QA_EINVAL   # plane without bit
    ok.flags = 4
    assert L.qa_denoise_guided_device(ctx._h, ptr[0], ptr[1], ptr[2], None, None, 7, 5, C.byref(ok), ptr[0], None) == QA_EINVAL
    ok.flags = 3
    assert L.qa_denoise_guided_device(ctx._h, None, ptr[1], ptr[2], ptr[3], ptr[4], 7, 5, C.byref(ok), ptr[0], None) == QA_EINVAL
    assert L.qa_denoise_guided_device(ctx._h, ptr[0], ptr[1], ptr[2], ptr[3], ptr[4], 7, 5, None, ptr[0], None) == QA_EINVAL
    assert L.qa_progressive_denoise_guided_device(ctx._h, C.byref(ok), ptr[0], None) != 0   # no progressive frame


def test_cli_denoise_guided_writes_the_fourth_image_and_leaves_the_three(tmp_path, ctx):
    from PIL import Image
    from qaray_amd import hip
    from qaray_amd.host import SCENES_DIR
    exe = os.path.join(ROOT, "qaray_amd", "lib", "qaray_hip")
    size = (48, 36)
    common = ["-batch", "-spp", "4", "-bounce", "5", "-size", str(size[0]), str(size[1]), "-root", SCENES_DIR]
    names = ("colorBuffer.png", "depthBuffer.png", "sampleBuffer.png")
    outs = {}
    for mode, extra in (("plain", []), ("den", ["-denoise"]), ("guided", ["-denoise-guided"]), ("guided3", ["-denoise-guided", "3"])):
        out = str(tmp_path / mode) + "_"
        r = subprocess.run([exe] + common + extra + ["-out", out, os.path.join(SCENES_DIR, TEXTURED)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
        outs[mode] = out
    ctx.upload_scene(blob(TEXTURED, size))
    region = (0, 0) + size
    rgb, depth, ns = ctx.render_region(region, 4, max_bounce=5)
    g = ctx.gbuffer(region)
    for mode in ("den", "guided", "guided3"):
        for png in names:
            with open(outs["plain"] + png, "rb") as a, open(outs[mode] + png, "rb") as b:
                assert a.read() == b.read(), (mode, png)
    image = lambda mode: np.asarray(Image.open(outs[mode] + "denoisedBuffer.png").convert("RGB"))
    shown = lambda x: hip.display_host(x, depth, ns, 4).color.reshape(size[1], size[0], 3)
    assert np.array_equal(image("den"), shown(hip.denoise_host(rgb, depth, ns)))   # -denoise alone is what it was
    assert np.array_equal(image("guided"), shown(hip.denoise_guided_host(rgb, depth, ns, g["normal"], g["albedo"])))
    assert np.array_equal(image("guided3"), shown(hip.denoise_guided_host(rgb, depth, ns, g["normal"], g["albedo"], iterations=3)))
    assert not np.array_equal(image("guided"), image("den"))
    r = subprocess.run([exe] + common + ["-denoise-guided", "-devices", "2", os.path.join(SCENES_DIR, TEXTURED)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True)
    assert r.returncode != 0 and "-denoise" in r.stdout and "-devices" in r.stdout
