"""The edge-avoiding filter on the device (qa_denoise_device, qa_progressive_denoise*: qa_denoise.hip): the device build of
qa_denoise_dev.h equals the host build (qa_test_denoise_host, pinned to a restatement of the specification by
tests/test_denoise_host.py) bit for bit, on plain frames and on progressive frames' slabs; the frame it reads is never changed;
the batch driver's -denoise writes a fourth image and leaves the other three alone."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, ensure_assets
from denoise_util import HOST_SIZES, bits, random_frame

pytestmark = pytest.mark.gpu

QA_EINVAL = -1
BOX = "example_project12_box.xml"
# (w, h): the host test's frames; one tile grid that fits; one that fits in neither dimension; long halos on one axis
SIZES = HOST_SIZES + ((64, 64), (67, 131), (16, 600), (600, 16))


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


def upload(rgb, depth, ns):
    import torch
    dev = torch.device("cuda", 0)
    return (torch.from_numpy(np.ascontiguousarray(rgb, np.float32)).to(dev), torch.from_numpy(np.ascontiguousarray(depth, np.float32)).to(dev),
            torch.from_numpy(np.ascontiguousarray(ns, np.uint32).view(np.int32)).to(dev))


def device_denoise(ctx, rgb, depth, ns, iterations, stream=None, alias=False):
    import torch
    t = upload(rgb, depth, ns)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    out = ctx.denoise_device(*t, out=t[0] if alias else None, iterations=iterations, stream=stream.cuda_stream if stream is not None else None)
    if stream is not None:
        stream.synchronize()
    else:
        ctx.synchronize()
    if not alias:   # the inputs are not written
        assert np.array_equal(bits(t[0].cpu().numpy()), bits(rgb))
    assert np.array_equal(bits(t[1].cpu().numpy()), bits(depth)) and np.array_equal(t[2].cpu().numpy().view(np.uint32), ns)
    return out.cpu().numpy()


@pytest.mark.parametrize("w,h", SIZES)
def test_device_equals_host_bit_for_bit(ctx, w, h):
    import torch
    from qaray_amd import hip
    rgb, depth, ns = random_frame(w, h, 100 * w + h)
    side = torch.cuda.Stream()
    for iterations in range(6):
        want = bits(hip.denoise_host(rgb, depth, ns, iterations=iterations))
        for stream in (None, side):
            for alias in (False, True):
                got = bits(device_denoise(ctx, rgb, depth, ns, iterations, stream, alias))
                bad = np.argwhere(got != want)
                assert bad.size == 0, (iterations, stream is not None, alias, len(bad), bad[:5])


def test_growing_and_shrinking_never_reads_a_stale_plane():
    from qaray_amd import hip
    c = hip.Context(0)   # (its own context: the working planes start at the first frame's size)
    try:
        small, large = random_frame(16, 16, 1), random_frame(67, 131, 2)
        first = device_denoise(c, *small, 5)
        assert np.array_equal(bits(device_denoise(c, *large, 5)), bits(hip.denoise_host(*large)))
        assert np.array_equal(bits(device_denoise(c, *small, 5)), bits(first))
        assert np.array_equal(bits(first), bits(hip.denoise_host(*small)))
    finally:
        c.close()


def same(a, b):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32)) for x, y in zip(a, b))


def test_progressive_frames_are_filtered_from_their_slabs_and_not_changed(ctx):
    import torch
    from qaray_amd import hip
    size = (96, 64)
    region = (0, 0) + size
    ctx.upload_scene(blob(BOX, size))
    one = ctx.render_region(region, 32)
    with ctx.progressive(region, 32) as prog:   # no filter between the passes
        for s in (4, 16, 32):
            prog.advance(s)
        assert same(prog.read(), one)
    with ctx.progressive(region, 32) as prog:
        for s in (4, 16):
            prog.advance(s)
            want = hip.denoise_host(*prog.read())
            assert np.array_equal(bits(prog.denoise()), bits(want))
            out = prog.denoise_device()
            ctx.synchronize()
            assert np.array_equal(bits(out.cpu().numpy()), bits(want))
            side = torch.cuda.Stream()
            out = prog.denoise_device(iterations=2, stream=side.cuda_stream)
            side.synchronize()
            assert np.array_equal(bits(out.cpu().numpy()), bits(hip.denoise_host(*prog.read(), iterations=2)))
            assert np.array_equal(bits(prog.denoise(iterations=0)), bits(prog.read()[0]))
        prog.advance(32)
        prog.denoise()
        assert same(prog.read(), one)
    assert same(ctx.render_region(region, 32), one)


def test_a_stale_frame_is_served_as_read_serves_it_and_an_ended_one_refused(ctx):
    """include/qaray_hip.h: after a scene edit advance returns QA_EINVAL until a restart, while read / display / status keep serving
    the old frame's pixels - and so does denoise; on a frame that has ended every qa_progressive_* call returns QA_EINVAL."""
    from qaray_amd import hip
    size = (96, 64)
    b = blob(BOX, size)
    ctx.upload_scene(b)
    prog = ctx.progressive((0, 0) + size, 16)
    prog.advance(4)
    before = prog.denoise()
    cam = hip.blob_camera(b.copy()).copy()
    cam["cam_pos"] = cam["cam_pos"] + np.float32(0.25)
    ctx.edit_camera(cam)
    with pytest.raises(hip.HipError) as e:
        prog.advance(8)
    assert e.value.code == QA_EINVAL
    assert np.array_equal(bits(prog.denoise()), bits(before))
    assert np.array_equal(bits(before), bits(hip.denoise_host(*prog.read())))
    prog.restart()
    prog.advance(4)
    assert np.array_equal(bits(prog.denoise()), bits(hip.denoise_host(*prog.read())))
    assert not np.array_equal(bits(prog.denoise()), bits(before))
    ctx.upload_scene(b)   # ends the frame
    with pytest.raises(hip.HipError) as e:
        prog.read()
    said = str(e.value)
    for call in (prog.denoise, prog.denoise_device):
        with pytest.raises(hip.HipError) as e:
            call()
        assert e.value.code == QA_EINVAL and str(e.value) == said
    prog.close()


def test_skipped_tiles_come_out_zero_and_weigh_nothing(ctx):
    from qaray_amd import hip
    size = (96, 64)
    ctx.upload_scene(blob(BOX, size))
    try:
        with ctx.progressive((0, 0) + size, 16) as prog:
            ctx.set_option("progressive_tile_limit", 37)
            prog.advance(4)
            rgb, depth, ns = prog.read()
            skipped = ns == 0
            assert skipped.sum() == (96 * 64 // 64 - 37) * 64
            out = prog.denoise()
            assert (bits(out)[skipped] == 0).all()
            assert np.array_equal(bits(out), bits(hip.denoise_host(rgb, depth, ns)))
            assert (out[~skipped] != rgb[~skipped]).any()
    finally:
        ctx.set_option("progressive_tile_limit", 0)


def test_invalid_arguments_are_refused(ctx):
    from qaray_amd import hip
    t = upload(*random_frame(7, 5, 3))
    for kw in ({"iterations": -1}, {"iterations": 7}, {"sigma_color": 0.0}, {"sigma_depth": float("nan")}, {"sigma_color": float("inf")}):
        with pytest.raises(hip.HipError) as e:
            ctx.denoise_device(*t, **kw)
        assert e.value.code == QA_EINVAL, kw
    p = hip.DenoiseParams.default()
    p.flags = 2
    with pytest.raises(hip.HipError) as e:
        ctx.denoise_device(*t, params=p)
    assert e.value.code == QA_EINVAL
    L, ok = hip.lib(), hip.DenoiseParams.default()
    import ctypes as C
    ptr = [x.data_ptr() for x in t]
    assert L.qa_denoise_device(ctx._h, None, ptr[1], ptr[2], 7, 5, C.byref(ok), ptr[0], None) == QA_EINVAL
    assert L.qa_denoise_device(ctx._h, ptr[0], ptr[1], ptr[2], 7, 5, C.byref(ok), None, None) == QA_EINVAL
    assert L.qa_denoise_device(ctx._h, ptr[0], ptr[1], ptr[2], 0, 5, C.byref(ok), ptr[0], None) == QA_EINVAL
    assert L.qa_denoise_device(ctx._h, ptr[0], ptr[1], ptr[2], 7, 5, None, ptr[0], None) == QA_EINVAL


def test_display_of_a_denoised_preview(ctx):
    """The README's recipe: denoise_device, then display_device of the result with the frame's depth and sample counts."""
    from qaray_amd import hip
    size = (96, 64)
    ctx.upload_scene(blob(BOX, size))
    rgb, depth, ns = ctx.render_region((0, 0) + size, 4)
    t = upload(rgb, depth, ns)
    denoised = ctx.denoise_device(*t)
    out = ctx.display_device(denoised, t[1], t[2], 4)
    ctx.synchronize()
    want = hip.display_host(hip.denoise_host(rgb, depth, ns), depth, ns, 4)
    for k in ("color", "count", "zimg", "countimg", "mask"):
        assert np.array_equal(out[k].cpu().numpy(), getattr(want, k)), k
    raw = hip.display_host(rgb, depth, ns, 4)
    assert not np.array_equal(want.color, raw.color)


def test_cli_denoise_writes_a_fourth_image_and_leaves_the_three(tmp_path, ctx):
    from PIL import Image
    from qaray_amd import hip
    from qaray_amd.host import SCENES_DIR
    exe = os.path.join(ROOT, "qaray_amd", "lib", "qaray_hip")
    size = (48, 36)
    common = ["-batch", "-spp", "4", "-bounce", "5", "-size", str(size[0]), str(size[1]), "-root", SCENES_DIR]
    names = ("colorBuffer.png", "depthBuffer.png", "sampleBuffer.png")
    outs = {}
    for mode, extra in (("plain", []), ("den", ["-denoise"]), ("den3", ["-denoise", "3"]), ("prog", ["-denoise", "-progressive", "2"])):
        out = str(tmp_path / mode) + "_"
        r = subprocess.run([exe] + common + extra + ["-out", out, os.path.join(SCENES_DIR, BOX)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
        outs[mode] = out
    assert not os.path.exists(outs["plain"] + "denoisedBuffer.png")
    ctx.upload_scene(blob(BOX, size))
    rgb, depth, ns = ctx.render_region((0, 0) + size, 4, max_bounce=5)
    for mode, iterations in (("den", None), ("den3", 3), ("prog", None)):
        for png in names:
            with open(outs["plain"] + png, "rb") as a, open(outs[mode] + png, "rb") as b:
                assert a.read() == b.read(), (mode, png)
        want = hip.display_host(hip.denoise_host(rgb, depth, ns, iterations=iterations), depth, ns, 4).color.reshape(size[1], size[0], 3)
        got = np.asarray(Image.open(outs[mode] + "denoisedBuffer.png").convert("RGB"))
        assert np.array_equal(got, want), mode
    plain = np.asarray(Image.open(outs["plain"] + "colorBuffer.png").convert("RGB"))
    assert not np.array_equal(np.asarray(Image.open(outs["den"] + "denoisedBuffer.png").convert("RGB")), plain)
    r = subprocess.run([exe] + common + ["-denoise", "-devices", "2", os.path.join(SCENES_DIR, BOX)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode != 0 and "-denoise" in r.stdout and "-devices" in r.stdout
