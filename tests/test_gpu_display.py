"""The FrameBuffer's 8-bit products computed on the device (qa_display_device, qa_progressive_display*: qa_display.hip): the device
build of qa_display_dev.h equals the host build (qa_test_display_host, pinned to the reference and to the host FrameBuffer by
tests/test_display_host.py) bit for bit; rendered and progressive frames' products equal FrameBuffer(deposit(...)) of the same
floats; the batch driver's progressive run leaves the one-shot run's images and FrameBuffer."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, bits, ensure_assets, golden_blob, load_golden
from test_display_host import edge_frames, random_sweep, same_stats

pytestmark = pytest.mark.gpu

QA_EINVAL = -1
PRODUCTS = ("color", "count", "zimg", "countimg", "mask")


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


def device_equals_host(ctx, rgb, depth, ns, spp_max, srgb, want, stream=None):
    """qa_display_device of the frame = qa_test_display_host of it: the wanted products and the statistics, bitwise; the products
    not wanted are not made."""
    import torch
    from qaray_amd import hip
    host = hip.display_host(rgb, depth, ns, spp_max, srgb=srgb)
    t = upload(rgb, depth, ns)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    out = ctx.display_device(*t, spp_max, srgb=srgb, want=want, stream=stream.cuda_stream if stream is not None else None)
    if stream is not None:
        stream.synchronize()
    else:
        ctx.synchronize()
    for k in PRODUCTS:
        if k in want:
            got = out[k].cpu().numpy()
            bad = np.flatnonzero(got != getattr(host, k))
            assert bad.size == 0, (k, srgb, bad[:5], got[bad[:5]], getattr(host, k)[bad[:5]])
        else:
            assert out[k] is None
    if "stats" in want:
        st = hip.stats_from_tensor(out["stats"])
        assert same_stats(st, host.stats), (st, host.stats)


@pytest.mark.parametrize("srgb", [True, False])
def test_device_equals_host_on_edge_frames(ctx, srgb):
    from qaray_amd import hip
    for name, (rgb, depth, ns, spp_max) in sorted(edge_frames().items()):
        try:
            device_equals_host(ctx, rgb, depth, ns, spp_max, srgb, hip.DISPLAY_ALL)
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}") from e


@pytest.mark.parametrize("want", [("color",), ("color", "stats"), ("zimg", "countimg"), ("count", "mask", "stats"), ("stats",),
                                  ("color", "count", "zimg", "countimg", "mask", "stats")])
def test_null_outputs(ctx, want):
    for name in ("skipped_pixels", "special_colours", "1026_pixels", "7_pixels"):
        rgb, depth, ns, spp_max = edge_frames()[name]
        device_equals_host(ctx, rgb, depth, ns, spp_max, True, want)


@pytest.mark.parametrize("srgb", [True, False])
def test_device_equals_host_on_a_random_sweep(ctx, srgb):
    from qaray_amd import hip
    rgb, depth, ns, spp_max = random_sweep()
    device_equals_host(ctx, rgb, depth, ns, spp_max, srgb, hip.DISPLAY_ALL)


def test_two_streams(ctx):
    """Calls on two streams of the caller's, alternating: the context's statistics block is one, so each waits for the last."""
    import torch
    from qaray_amd import hip
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    frames = edge_frames()
    for k, name in enumerate(("4103_pixels", "spp_max_2048", "special_depths", "1021_pixels", "special_colours", "skipped_pixels")):
        rgb, depth, ns, spp_max = frames[name]
        device_equals_host(ctx, rgb, depth, ns, spp_max, bool(k & 2), hip.DISPLAY_ALL, stream=(s1, s2)[k & 1])
    # both in flight before either is read
    a, b = frames["4103_pixels"], random_sweep(1 << 18, seed=11)
    ta, tb = upload(*a[:3]), upload(*b[:3])
    torch.cuda.synchronize()
    oa = ctx.display_device(*ta, a[3], stream=s1.cuda_stream)
    ob = ctx.display_device(*tb, b[3], stream=s2.cuda_stream)
    s1.synchronize(); s2.synchronize()
    for out, f in ((oa, a), (ob, b)):
        host = hip.display_host(*f[:3], f[3])
        assert all(np.array_equal(out[k].cpu().numpy(), getattr(host, k)) for k in PRODUCTS)
        assert same_stats(hip.stats_from_tensor(out["stats"]), host.stats)


def test_unaligned_buffers_take_the_tail_path(ctx):
    """Views that start 4 bytes (inputs) / 1 byte (outputs) into their tensors: every pixel goes the one-by-one way."""
    import torch
    from qaray_amd import hip
    rgb, depth, ns, spp_max = edge_frames()["1026_pixels"]
    n = depth.size
    dev = torch.device("cuda", 0)
    t = upload(np.concatenate([np.zeros(1, np.float32), rgb.ravel()]), np.concatenate([np.zeros(1, np.float32), depth]),
               np.concatenate([np.zeros(1, np.uint32), ns]))
    color = torch.zeros(3 * n + 1, dtype=torch.uint8, device=dev)
    zimg = torch.zeros(n + 1, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    out = ctx.display_device(t[0][1:], t[1][1:], t[2][1:], spp_max, want=("count", "stats"), color=color[1:], zimg=zimg[1:])
    ctx.synchronize()
    host = hip.display_host(rgb, depth, ns, spp_max)
    assert np.array_equal(out["color"].cpu().numpy(), host.color) and np.array_equal(out["zimg"].cpu().numpy(), host.zimg)
    assert np.array_equal(out["count"].cpu().numpy(), host.count) and same_stats(hip.stats_from_tensor(out["stats"]), host.stats)
    assert int(color[0]) == 0 and int(zimg[0]) == 0


def framebuffer_products(rgb, depth, ns, spp_max, srgb):
    from qaray_amd.host import FrameBuffer
    h, w = depth.shape
    fb = FrameBuffer(w, h)
    fb.deposit(0, 0, w, h, rgb, depth, ns, spp_max, use_srgb=srgb)
    out = {"color": fb.pixels, "count": fb.sample_count, "zimg": fb.z_image, "countimg": fb.sample_count_image, "mask": fb.mask}
    fb.close()
    return out


def _eightbit_names():
    d = os.path.join(GOLDEN, "eightbit")
    return sorted(f[:-4] for f in os.listdir(d) if f.endswith(".npz"))


@pytest.mark.parametrize("name", _eightbit_names())
def test_rendered_frames(ctx, name):
    """render_region_device then display_device, nothing leaving the device in between, = FrameBuffer(deposit(...)) of the same floats,
    byte for byte.  Against the reference's own products: z image and count image exact; colour exact on the Cornell box, elsewhere
    within the rule of test_cli_pngs_equal_the_references_8bit_products (the radiance's margin: at most one level on at most 0.2 %
    of the bytes)."""
    import torch
    z = np.load(os.path.join(GOLDEN, "eightbit", name + ".npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    w, h = meta["width"], meta["height"]
    ctx.upload_scene(blob(meta["scene"], (w, h)))
    dev = torch.device("cuda", 0)
    rgb = torch.zeros((h, w, 3), dtype=torch.float32, device=dev)
    depth = torch.zeros((h, w), dtype=torch.float32, device=dev)
    ns = torch.zeros((h, w), dtype=torch.int32, device=dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    ctx.render_region_device((0, 0, w, h), meta["spp_min"], rgb, depth, ns, seed=meta["seed"], spp_max=meta["spp_max"], stream=s.cuda_stream)
    out = ctx.display_device(rgb, depth, ns, meta["spp_max"], srgb=bool(meta["srgb"]), stream=s.cuda_stream)
    s.synchronize()
    ref = framebuffer_products(rgb.cpu().numpy(), depth.cpu().numpy(), ns.cpu().numpy().view(np.uint32), meta["spp_max"], bool(meta["srgb"]))
    got = {k: out[k].cpu().numpy().reshape(ref[k].shape) for k in PRODUCTS}
    for k in PRODUCTS:
        assert np.array_equal(got[k], ref[k]), k
    assert np.array_equal(got["zimg"], z["zimg"]) and np.array_equal(got["countimg"], z["countimg"])
    if "box" in name:
        assert np.array_equal(got["color"], z["color"])
    else:
        d = np.abs(got["color"].astype(np.int16) - z["color"].astype(np.int16))
        assert d.max() <= 1 and (d != 0).mean() <= 0.002, (int(d.max()), float((d != 0).mean()))


def display_equals_deposit_of_read(prog, spp_max, srgb=True):
    """Progressive.display() = FrameBuffer(deposit(read())), every product; -> (display, read)"""
    d = prog.display(srgb=srgb)
    frame = prog.read()
    ref = framebuffer_products(*frame, spp_max, srgb)
    for k in PRODUCTS:
        bad = np.argwhere(getattr(d, k) != ref[k])
        assert bad.size == 0, (k, bad[:5])
    return d, frame


def same(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


# an LDS-resident scene and a textured cooperative one
PROGRESSIVE = {"box": ("example_project12_box.xml", (96, 64), 64, "RES=1"), "object_textured": ("example_project7_object.xml", (80, 56), 16, "TEX=1")}


@pytest.mark.parametrize("case", sorted(PROGRESSIVE))
@pytest.mark.parametrize("srgb", [True, False])
def test_progressive_display_after_every_pass(ctx, case, srgb):
    """After every pass of 1, 4, 16, ... spp display() equals FrameBuffer(deposit(read())); display() between passes changes
    nothing (the final float frame is render_region's, bit for bit); the display after the last pass is the one-shot frame's."""
    import torch
    from qaray_amd import hip
    scene, size, n, kernel = PROGRESSIVE[case]
    ctx.upload_scene(blob(scene, size))
    region = (0, 0) + size
    with ctx.progressive(region, n) as prog:
        s = 1
        while True:
            prog.advance(min(s, n))
            d, frame = display_equals_deposit_of_read(prog, n, srgb)
            assert kernel in ctx.kernel_name(), ctx.kernel_name()
            if s >= n:
                break
            s *= 4
        dd = prog.display_device(srgb=srgb)
        ctx.synchronize()
        assert all(np.array_equal(dd[k].cpu().numpy().reshape(getattr(d, k).shape), getattr(d, k)) for k in PRODUCTS)
        assert same_stats(hip.stats_from_tensor(dd["stats"]), d.stats)
    one = ctx.render_region(region, n)
    assert same(frame, one)
    t = upload(*one)
    torch.cuda.synchronize()
    out = ctx.display_device(*t, n, srgb=srgb)
    ctx.synchronize()
    assert all(np.array_equal(out[k].cpu().numpy().reshape(getattr(d, k).shape), getattr(d, k)) for k in PRODUCTS)
    assert same_stats(hip.stats_from_tensor(out["stats"]), d.stats)


def test_progressive_display_of_an_adaptive_frame(ctx):
    """The adaptive sphere frame (4 to 32 spp): finished and unfinished pixels side by side in every preview."""
    rgb, depth, ns, meta = load_golden("sphere_adaptive_64x48_4to32spp")
    ctx.upload_scene(golden_blob(meta))
    region = tuple(meta["crop"])
    mixed = 0
    with ctx.progressive(region, meta["spp_min"], spp_max=meta["spp_max"], max_bounce=meta["bounce"], seed=meta["seed"]) as prog:
        for s in (1, 4, 5, 8, 16, 32):
            prog.advance(s)
            d, frame = display_equals_deposit_of_read(prog, meta["spp_max"], srgb=False)
            st = prog.status()
            mixed += 0 < st["pixels_finished"] < ns.size
    assert mixed >= 1
    assert np.array_equal(frame[2], ns) and np.array_equal(bits(frame[1]), bits(depth))


def test_progressive_display_after_a_pass_cut_short(ctx):
    """progressive_tile_limit: pixels no pass has reached have ns == 0 - colour 0, count 0, depth 0.0f in zmin, mask = (ns != 0)."""
    size = (64, 48)
    ctx.upload_scene(blob("example_project3_sphere.xml", size))
    region = (0, 0) + size
    try:
        with ctx.progressive(region, 8) as prog:
            ctx.set_option("progressive_tile_limit", 10)
            prog.advance(4)
            d, frame = display_equals_deposit_of_read(prog, 8)
            assert np.array_equal(d.mask, (frame[2] != 0).astype(np.uint8)) and 0 < d.mask.sum() == 10 * 64
            assert d.stats["zmin"] == 0.0 and (d.color[d.mask == 0] == 0).all()
            ctx.set_option("progressive_tile_limit", 0)
            prog.advance(4)
            d, frame = display_equals_deposit_of_read(prog, 8)
            assert d.mask.all()
            prog.advance(8)
            display_equals_deposit_of_read(prog, 8)
            final = prog.read()
    finally:
        ctx.set_option("progressive_tile_limit", 0)
    assert same(final, ctx.render_region(region, 8))


def test_errors(ctx):
    import torch
    from qaray_amd import hip
    L = hip.lib()
    rgb, depth, ns, spp_max = edge_frames()["skipped_pixels"]
    t = upload(rgb, depth, ns)
    out = torch.zeros(3 * depth.size, dtype=torch.uint8, device=t[0].device)
    torch.cuda.synchronize()
    args = (t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
    outs = (out.data_ptr(), None, None, None, None, None, None)
    assert L.qa_display_device(ctx._h, *args, 0, 4, 1, *outs) == QA_EINVAL            # zero pixels
    assert L.qa_display_device(ctx._h, *args, depth.size, 0, 1, *outs) == QA_EINVAL   # spp_max = 0
    assert L.qa_display_device(ctx._h, None, t[1].data_ptr(), t[2].data_ptr(), depth.size, 4, 1, *outs) == QA_EINVAL   # no source buffer
    assert L.qa_display_device(None, *args, depth.size, 4, 1, *outs) == QA_EINVAL
    # a frame that was ended: what the other qa_progressive_* calls say
    ctx.upload_scene(blob("example_project3_sphere.xml", (64, 48)))
    prog = ctx.progressive((0, 0, 64, 48), 4)
    prog.advance(1)
    prog.display()
    ctx.upload_scene(blob("example_project12_box.xml", (64, 48)))
    with pytest.raises(hip.HipError) as e:
        prog.read()
    said = str(e.value)
    with pytest.raises(hip.HipError) as e:
        prog.display()
    assert e.value.code == QA_EINVAL and str(e.value) == said and "scene" in said
    with pytest.raises(hip.HipError) as e:
        prog.display_device()
    assert e.value.code == QA_EINVAL and str(e.value) == said
    prog.close()
    with pytest.raises(hip.HipError) as e:   # no frame at all
        hip.Progressive(ctx, (0, 0, 64, 48)).display()
    assert e.value.code == QA_EINVAL


@pytest.mark.parametrize("scene,size,spp,srgb", [("example_project12_box.xml", (96, 64), 64, 1), ("example_project7_object.xml", (80, 56), 32, 0)])
def test_cli_progressive_pngs_equal_the_one_shot_runs(tmp_path, scene, size, spp, srgb):
    """-progressive: every pass's PNGs now come from qa_progressive_display; the final ones are the one-shot run's, byte for byte."""
    from qaray_amd.host import SCENES_DIR
    ensure_assets()
    exe = os.path.join(ROOT, "qaray_amd", "lib", "qaray_hip")
    common = ["-batch", "-spp", str(spp), "-srgb", str(srgb), "-size", str(size[0]), str(size[1]), "-root", SCENES_DIR]
    outs = {}
    for mode, extra in (("one", []), ("prog", ["-progressive", "16"])):
        out = str(tmp_path / mode) + "_"
        r = subprocess.run([exe] + common + extra + ["-out", out, os.path.join(SCENES_DIR, scene)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
        outs[mode] = (out, r.stdout)
    passes = [l for l in outs["prog"][1].splitlines() if l.startswith("pass to ")]
    assert len(passes) == spp // 16 and all(" spp reached, " in l and l.endswith(" ms") for l in passes), outs["prog"][1]
    for png in ("colorBuffer.png", "depthBuffer.png", "sampleBuffer.png"):
        with open(outs["one"][0] + png, "rb") as a, open(outs["prog"][0] + png, "rb") as b:
            assert a.read() == b.read(), png


def test_cli_progressive_leaves_the_one_shot_framebuffer(tmp_path):
    """tests/cpp/progressive_fb_state.cpp: the batch driver's Renderer, progressive and one-shot, in one process - the FrameBuffers
    they leave (colour, z buffer floats, count, mask, both images) are the same; the rendered pixels are counted once per pass."""
    from qaray_amd.host import SCENES_DIR
    csrc = os.path.join(ROOT, "qaray_amd", "csrc")
    lib = os.path.join(ROOT, "qaray_amd", "lib")
    exe = str(tmp_path / "progressive_fb_state")
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O2", "-pthread", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(csrc, "host"), os.path.join(ROOT, "tests", "cpp", "progressive_fb_state.cpp"),
                    os.path.join(csrc, "host", "renderer.cpp"), "-L" + lib, "-lqaray_host", "-lqaray_hip", "-Wl,-rpath," + lib, "-o", exe], check=True)
    for scene, spp, step in (("example_project3_sphere.xml", 40, 16), ("example_project12_box.xml", 16, 16)):
        r = subprocess.run([exe, os.path.join(SCENES_DIR, scene), SCENES_DIR, "96", "64", str(spp), str(step), str(tmp_path) + "/"],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0 and "same as the one-shot run's" in r.stdout, r.stdout
