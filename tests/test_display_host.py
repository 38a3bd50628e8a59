"""The 8-bit products of qa_display_dev.h on the CPU (qa_test_display_host: the source the device kernels are compiled from, built
for the host) against the reference's own bytes (tests/golden/eightbit) and against the host FrameBuffer (Deposit +
ComputeZBufferImage + ComputeSampleCountImage), byte for byte.  tests/test_gpu_display.py pins the device build to this one."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, bits
from qaray_amd import hip
from qaray_amd.host import FrameBuffer

MISS = np.float32(1.0e30)


def _eightbit_names():
    d = os.path.join(GOLDEN, "eightbit")
    return sorted(f[:-4] for f in os.listdir(d) if f.endswith(".npz"))


@pytest.mark.parametrize("name", _eightbit_names())
def test_display_host_equals_the_references_own_bytes(name):
    """Its inputs are the reference's own floats, its expected outputs the reference's own 8-bit arrays: no tolerance."""
    z = np.load(os.path.join(GOLDEN, "eightbit", name + ".npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    d = hip.display_host(z["rgb"], z["depth"], z["ns"], meta["spp_max"], srgb=bool(meta["srgb"]))
    h, w = meta["height"], meta["width"]
    assert np.array_equal(d.color.reshape(h, w, 3), z["color"])
    assert np.array_equal(d.count.reshape(h, w), z["count"])
    assert np.array_equal(d.zimg.reshape(h, w), z["zimg"])
    assert np.array_equal(d.countimg.reshape(h, w), z["countimg"])
    assert (d.mask == 1).all()


def expected_stats(depth, ns, count):
    """What the sequential loops of ComputeZBufferImage / ComputeSampleCountImage end with (the FrameBuffer keeps them in locals):
    zmin from 1e30 down, zmax from 0 up over the depths other than 1e30, NaNs never counting, a skipped pixel's depth being 0;
    a zero zmin is reported as +0."""
    z = np.where(ns.ravel() != 0, depth.ravel(), np.float32(0)).astype(np.float32)
    z = z[(z != MISS) & ~np.isnan(z)]
    zmin = min(MISS, z.min()) if z.size else MISS
    zmax = max(np.float32(0), z.max()) if z.size else np.float32(0)
    zmin = np.float32(0) if zmin == 0 else np.float32(zmin)
    zmax = np.float32(0) if zmax == 0 else np.float32(zmax)
    return {"zmin": float(zmin), "zmax": float(zmax), "smin": min(255, int(count.min())), "smax": max(0, int(count.max()))}


def same_stats(a, b):
    fa = np.array([a["zmin"], a["zmax"]], np.float32)
    fb_ = np.array([b["zmin"], b["zmax"]], np.float32)
    return np.array_equal(bits(fa), bits(fb_)) and a["smin"] == b["smin"] and a["smax"] == b["smax"]


def check_against_framebuffer(rgb, depth, ns, spp_max, srgb, what=("color", "count", "zimg", "countimg", "mask")):
    """display_host of a frame equals FrameBuffer(Init + deposit + the two images) of it, every product and the statistics."""
    rgb = np.ascontiguousarray(rgb, np.float32).reshape(-1, 3)
    depth = np.ascontiguousarray(depth, np.float32).ravel()
    ns = np.ascontiguousarray(ns, np.uint32).ravel()
    n = depth.size
    fb = FrameBuffer(n, 1)
    fb.deposit(0, 0, n, 1, rgb, depth, ns, spp_max, use_srgb=srgb)
    ref = {"color": fb.pixels.ravel(), "count": fb.sample_count.ravel(), "zimg": fb.z_image.ravel(),
           "countimg": fb.sample_count_image.ravel(), "mask": fb.mask.ravel()}
    fb.close()
    d = hip.display_host(rgb, depth, ns, spp_max, srgb=srgb)
    for k in what:
        got = getattr(d, k)
        bad = np.flatnonzero(got != ref[k])
        assert bad.size == 0, (k, srgb, bad[:5], got[bad[:5]], ref[k][bad[:5]])
    st = expected_stats(depth, ns, ref["count"])
    assert same_stats(d.stats, st), (d.stats, st)
    return d


def f32(*v):
    return np.array(v, np.float32)


def special_colours():
    """NaN, +-inf, negative, -0, denormals, the sRGB knee and its two neighbours, values that land on x.5 after * 255 and their
    neighbours, values around 1."""
    knee = np.float32(0.0031308)
    v = [np.nan, np.inf, -np.inf, -1.0, -1e-30, -0.0, 0.0, 1e-45, 1e-40, -1e-40, 1.17549435e-38, knee, np.nextafter(knee, np.float32(0)),
         np.nextafter(knee, np.float32(1)), 1.0, np.nextafter(np.float32(1), np.float32(0)), np.nextafter(np.float32(1), np.float32(2)), 2.0,
         1e30, 3.4e38, 0.5, 0.25, 1.0 / 255.0]
    half = (np.arange(256, dtype=np.float64) + 0.5) / 255.0
    for h in half.astype(np.float32):
        v += [h, np.nextafter(h, np.float32(0)), np.nextafter(h, np.float32(1))]
    # the linear values whose sRGB image lies at x.5: the inverse of LinearToSRGB in double, and the floats around it
    s = half[half <= 1.0]
    lin = np.where(s < 12.92 * 0.0031308, s / 12.92, ((s + 0.055) / 1.055) ** 2.4).astype(np.float32)
    for x in lin:
        y = x
        for _ in range(3):
            y = np.nextafter(y, np.float32(0))
        for _ in range(7):
            v.append(y)
            y = np.nextafter(y, np.float32(2))
    v = np.array(v, np.float32)
    return np.concatenate([v, np.array([0x7FC00001, 0xFFC00000, 0x7F800001, 0x80000001, 0x007FFFFF], np.uint32).view(np.float32)])


def edge_frames():
    """name -> (rgb[n,3], depth[n], ns[n], spp_max): the frames the device test (tests/test_gpu_display.py) runs as well."""
    rng = np.random.default_rng(20240517)
    frames = {}

    def colours(n):
        return rng.random((n, 3), dtype=np.float32) * np.float32(1.2)

    n = 37
    frames["all_miss"] = (colours(n), np.full(n, MISS), np.full(n, 4, np.uint32), 4)
    frames["zmax_equals_zmin"] = (colours(n), np.full(n, np.float32(3.25)), np.full(n, 4, np.uint32), 4)
    frames["zmax_equals_zmin_with_misses"] = (colours(n), np.where(np.arange(n) % 3 == 0, MISS, np.float32(7.5)).astype(np.float32), np.full(n, 2, np.uint32), 4)
    ns = rng.integers(0, 5, 101).astype(np.uint32)
    ns[:3] = 0
    frames["skipped_pixels"] = (colours(101), (rng.random(101, dtype=np.float32) * 20 + 1).astype(np.float32), ns, 4)
    frames["all_skipped"] = (colours(9), np.full(9, np.float32(5)), np.zeros(9, np.uint32), 4)
    sc = special_colours()
    m = (sc.size + 2) // 3 * 3
    c = np.resize(sc, m).reshape(-1, 3)
    frames["special_colours"] = (c, (rng.random(c.shape[0], dtype=np.float32) * 10).astype(np.float32), np.full(c.shape[0], 3, np.uint32), 4)
    zs = f32(-1.0, -0.0, 0.0, np.inf, -np.inf, np.nan, 1e30, 1e-40, -3e38, 3e38, 2.0, 5.0, np.nextafter(MISS, np.float32(0)), np.nextafter(MISS, np.float32(np.inf)))
    frames["special_depths"] = (colours(zs.size), zs, np.full(zs.size, 1, np.uint32), 2)
    frames["depth_zero_signs"] = (colours(5), f32(0.0, -0.0, 4.0, -0.0, 0.0), np.full(5, 1, np.uint32), 1)
    frames["depth_negative_zero_first"] = (colours(4), f32(-0.0, 0.0, 1.0, 2.0), np.full(4, 1, np.uint32), 1)
    frames["depth_inf_only"] = (colours(6), f32(np.inf, np.inf, 1e30, np.inf, np.inf, np.inf), np.full(6, 1, np.uint32), 1)
    frames["depth_nan_only"] = (colours(5), f32(*[np.nan] * 5), np.full(5, 1, np.uint32), 1)
    frames["depth_negative_only"] = (colours(7), f32(-1, -2, -3, -np.inf, -5, -6, -7), np.full(7, 1, np.uint32), 1)
    frames["spp_max_1"] = (colours(64), (rng.random(64, dtype=np.float32) * 9).astype(np.float32), rng.integers(0, 2, 64).astype(np.uint32), 1)
    frames["spp_max_2048"] = (colours(4099), (rng.random(4099, dtype=np.float32) * 9).astype(np.float32), rng.integers(0, 2049, 4099).astype(np.uint32), 2048)
    frames["counts_all_equal"] = (colours(50), (rng.random(50, dtype=np.float32) * 9).astype(np.float32), np.full(50, 7, np.uint32), 16)
    frames["counts_beyond_spp_max"] = (colours(8), np.full(8, np.float32(2)), np.array([1, 5, 300, 70000, 2 ** 31, 2 ** 32 - 1, 16843010, 4], np.uint32), 4)
    frames["one_pixel"] = (f32(0.2, 0.5, 0.9).reshape(1, 3), f32(4.0), np.array([4], np.uint32), 4)
    frames["one_pixel_miss"] = (f32(0.2, 0.5, 0.9).reshape(1, 3), f32(1e30), np.array([4], np.uint32), 4)
    for k in (2, 3, 5, 6, 7, 1021, 1026, 4103):   # pixel counts not divisible by 4
        frames[f"{k}_pixels"] = (colours(k), np.where(rng.random(k) < 0.2, MISS, rng.random(k, dtype=np.float32) * 30).astype(np.float32),
                                 rng.integers(0, 9, k).astype(np.uint32), 8)
    return frames


def random_sweep(n=1 << 20, seed=7):
    """>= 10^6 pixels: colours uniform around [0, 1], some of any bit pattern; depths with misses, zeros and NaNs; counts 0..spp."""
    rng = np.random.default_rng(seed)
    rgb = (rng.random((n, 3), dtype=np.float32) * np.float32(1.3) - np.float32(0.05)).astype(np.float32)
    anyb = rng.random((n, 3)) < 0.05
    rgb[anyb] = rng.integers(0, 2 ** 32, int(anyb.sum()), dtype=np.uint64).astype(np.uint32).view(np.float32)
    small = rng.random((n, 3)) < 0.05
    rgb[small] = (rng.random(int(small.sum()), dtype=np.float32) * np.float32(0.007)).astype(np.float32)
    depth = (rng.random(n, dtype=np.float32) * np.float32(40) + np.float32(0.5)).astype(np.float32)
    depth[rng.random(n) < 0.2] = MISS
    odd = rng.random(n) < 0.001   # (inside the range, so that the z image keeps its levels; the wild depths are in edge_frames)
    depth[odd] = rng.choice(np.array([0.0, -0.0, 1e-40, 0.25, np.nan, 40.5], np.float32), int(odd.sum()))
    ns = rng.integers(0, 65, n).astype(np.uint32)
    return rgb, depth, ns, 64


@pytest.mark.parametrize("name", sorted(edge_frames()))
@pytest.mark.parametrize("srgb", [True, False])
def test_display_host_equals_the_framebuffer_on_edge_frames(name, srgb):
    rgb, depth, ns, spp_max = edge_frames()[name]
    check_against_framebuffer(rgb, depth, ns, spp_max, srgb)


@pytest.mark.parametrize("srgb", [True, False])
def test_display_host_equals_the_framebuffer_on_a_random_sweep(srgb):
    rgb, depth, ns, spp_max = random_sweep()
    assert depth.size >= 10 ** 6
    d = check_against_framebuffer(rgb, depth, ns, spp_max, srgb)
    assert len(np.unique(d.color)) == 256 and len(np.unique(d.zimg)) > 200 and len(np.unique(d.countimg)) > 60


@pytest.mark.parametrize("srgb", [True, False])
def test_colour_byte_over_every_4099th_float(srgb):
    """Every 4099th of all 2^32 float bit patterns as a colour component, against the FrameBuffer (the full sweep, against
    framebuffer.cpp's expression built with the host libm: tests/cpp/display_exhaustive.c, quoted in DESIGN.md)."""
    x = np.arange(0, 2 ** 32, 4099, dtype=np.uint64).astype(np.uint32)
    x = np.resize(x, (x.size + 2) // 3 * 3).view(np.float32).reshape(-1, 3)
    n = x.shape[0]
    assert 3 * n >= 2 ** 32 // 4099
    check_against_framebuffer(x, np.full(n, np.float32(1)), np.full(n, 1, np.uint32), 1, srgb, what=("color",))


def test_display_exhaustive_tool_builds_and_agrees_on_a_strided_sweep(tmp_path):
    exe = str(tmp_path / "display_exhaustive")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fopenmp", os.path.join(ROOT, "tests", "cpp", "display_exhaustive.c"), "-o", exe,
                    "-ldl", "-lm"], check=True)
    r = subprocess.run([exe, hip.HIP_LIB_PATH, "509"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and " 0 mismatches" in r.stdout, r.stdout


def test_null_outputs_and_bad_arguments():
    import ctypes as C
    rgb, depth, ns, spp_max = edge_frames()["skipped_pixels"]
    n = depth.size
    full = hip.display_host(rgb, depth, ns, spp_max)
    L = hip.lib()
    color = np.zeros(3 * n, np.uint8)
    args = (np.ascontiguousarray(rgb).ctypes.data, depth.ctypes.data, ns.ctypes.data)
    assert L.qa_test_display_host(*args, n, spp_max, 1, color.ctypes.data, None, None, None, None, None) == 0
    assert np.array_equal(color, full.color)
    st = hip.DisplayStats()
    assert L.qa_test_display_host(*args, n, spp_max, 1, None, None, None, None, None, C.addressof(st)) == 0
    assert same_stats(st.as_dict(), full.stats)
    assert L.qa_test_display_host(*args, 0, spp_max, 1, color.ctypes.data, None, None, None, None, None) == -1     # QA_EINVAL
    assert L.qa_test_display_host(*args, n, 0, 1, color.ctypes.data, None, None, None, None, None) == -1
    assert L.qa_test_display_host(None, depth.ctypes.data, ns.ctypes.data, n, spp_max, 1, color.ctypes.data, None, None, None, None, None) == -1


@pytest.mark.parametrize("with_depth", [True, False])
def test_framebuffer_adopts_products_as_deposit_leaves_them(with_depth):
    """FrameBuffer::AdoptProducts of a whole frame's products = Deposit + the two images of the same floats: colour, count, mask, the
    rendered-pixel count (and the z buffer's floats where mask is set, when the depth comes along)."""
    w, h = 23, 11
    rng = np.random.default_rng(3)
    rgb = rng.random((h, w, 3), dtype=np.float32)
    depth = np.where(rng.random((h, w)) < 0.3, MISS, rng.random((h, w), dtype=np.float32) * 9 + 1).astype(np.float32)
    ns = rng.integers(0, 5, (h, w)).astype(np.uint32)
    ref = FrameBuffer(w, h)
    ref.deposit(0, 0, w, h, rgb, depth, ns, 4, use_srgb=True)
    d = hip.display_host(rgb, depth, ns, 4, srgb=True)
    fb = FrameBuffer(w, h)
    fb.adopt_products(d.color, d.count, d.zimg, d.countimg, d.mask, depth if with_depth else None)
    assert np.array_equal(fb.pixels, ref.pixels) and np.array_equal(fb.sample_count, ref.sample_count) and np.array_equal(fb.mask, ref.mask)
    assert fb.num_rendered_pixels == ref.num_rendered_pixels == w * h
    if with_depth:
        assert np.array_equal(bits(fb.zbuffer), bits(ref.zbuffer))
        assert np.array_equal(fb.z_image, ref.z_image)
    else:
        assert (fb.zbuffer == 0).all()
    assert np.array_equal(fb.sample_count_image, ref.sample_count_image)
    fb.close(); ref.close()
