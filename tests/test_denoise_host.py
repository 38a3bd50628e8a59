"""The edge-avoiding filter of qa_denoise_dev.h on the CPU (qa_test_denoise_host: the source the device kernels are compiled from,
built for the host) against a float64 numpy restatement of the header's specification (tests/denoise_util.py), against the rules
the specification states exactly, and - for the one claim about quality - against the oracle's converged frame.
tests/test_gpu_denoise.py pins the device build to this one, bit for bit."""
import ctypes as C

import numpy as np
import pytest

from denoise_util import HIT, HOST_SIZES, MISS, MISS_CLASS, VOID, bits, classes, denoise_ref, luma, random_frame
from qaray_amd import hip


def ulp_distance(a, b):
    """The distance of finite float32 values in units in the last place (ordered integer keys)."""
    def key(x):
        u = bits(x).astype(np.int64)
        return np.where(u & 0x80000000, 0x80000000 - u, u)
    return np.abs(key(a) - key(b))


@pytest.mark.parametrize("w,h", HOST_SIZES)
def test_host_build_agrees_with_the_restatement(w, h):
    """Bound: 1e-4 of the frame's largest input component (5 iterations of about 30 fp32 roundings, 1e-5, times 10 for the
    sensitivity of the exponentials).  Measured: at most 2.8e-7 of it (33x17, one iteration); 8.5e-8 and less on the smaller
    frames.  At steps 8 and 16 almost every tap of the 7x5 frame falls outside the image."""
    rgb, depth, ns = random_frame(w, h, 100 * w + h)
    live = classes(rgb, depth, ns) != VOID
    top = float(np.max(np.where(np.isfinite(rgb), rgb, 0)))
    for iterations in range(6):
        got = hip.denoise_host(rgb, depth, ns, iterations=iterations)
        want = denoise_ref(rgb, depth, ns, iterations=iterations)
        assert np.array_equal(bits(got)[~live], bits(rgb)[~live])
        if live.any():
            dev = float(np.abs(got[live].astype(np.float64) - want[live]).max())
            print(f"{w}x{h} iterations {iterations}: deviation {dev / top:.3g} of the largest component")
            assert dev <= 1e-4 * top


def test_zero_iterations_return_the_input_bits_and_inputs_are_not_modified():
    rgb, depth, ns = random_frame(33, 17, 7)
    keep = rgb.copy(), depth.copy(), ns.copy()
    assert np.array_equal(bits(hip.denoise_host(rgb, depth, ns, iterations=0)), bits(rgb))
    hip.denoise_host(rgb, depth, ns)
    assert np.array_equal(bits(rgb), bits(keep[0])) and np.array_equal(bits(depth), bits(keep[1])) and np.array_equal(ns, keep[2])


def test_void_pixels_pass_through_and_weigh_nothing():
    rgb, depth, ns = random_frame(33, 17, 11)
    void = classes(rgb, depth, ns) == VOID
    assert (ns == 0).any() and np.isnan(rgb).any() and np.isinf(rgb).any() and void.sum() > 20
    out = hip.denoise_host(rgb, depth, ns)
    assert np.array_equal(bits(out)[void], bits(rgb)[void])
    assert np.isfinite(out[~void]).all()
    # another colour in every void pixel that stays void with it: any finite colour where ns == 0, another non-finite one elsewhere
    other = rgb.copy()
    skipped = ns == 0
    other[skipped] = np.float32(123.0)
    other[void & ~skipped] = np.float32([np.inf, -np.inf, np.nan])
    assert np.array_equal(classes(other, depth, ns) == VOID, void)
    out2 = hip.denoise_host(other, depth, ns)
    assert np.array_equal(bits(out2)[~void], bits(out)[~void])
    assert np.array_equal(bits(out2)[void], bits(other)[void])


def test_hit_and_miss_pixels_in_a_checkerboard_never_mix():
    """Every output is its own colour plus a convex combination of differences to pixels of its class, so it lies in the closed
    range of its class's inputs per channel.  Slack: one rounding of the division, 2^-24 of the largest component.  Measured
    excursion outside the range: 0."""
    w, h = 24, 20
    r = np.random.default_rng(5)
    y, x = np.mgrid[0:h, 0:w]
    miss = (x + y) % 2 == 1
    rgb = np.where(miss[..., None], 5 + r.random((h, w, 3)), r.random((h, w, 3))).astype(np.float32)   # miss 5 .. 6, hit 0 .. 1
    depth = np.where(miss, MISS, 4 + 0.1 * x).astype(np.float32)
    ns = np.ones((h, w), np.uint32)
    cls = classes(rgb, depth, ns)
    assert (cls[miss] == MISS_CLASS).all() and (cls[~miss] == HIT).all()
    out = hip.denoise_host(rgb, depth, ns)
    slack = 2.0 ** -24 * float(rgb.max())
    for m in (miss, ~miss):
        for ch in range(3):
            assert out[..., ch][m].min() >= rgb[..., ch][m].min() - slack and out[..., ch][m].max() <= rgb[..., ch][m].max() + slack
    assert np.abs(out - rgb).max() > 0.05   # (and the filter did something)


def test_constant_colour_on_a_slanted_plane_stays_constant():
    w, h = 40, 24
    y, x = np.mgrid[0:h, 0:w]
    rgb = np.empty((h, w, 3), np.float32)
    rgb[:] = np.float32([0.3, 0.7, 1.9])
    depth = (2 + 0.37 * x + 0.11 * y).astype(np.float32)
    out = hip.denoise_host(rgb, depth, np.full((h, w), 4, np.uint32))
    assert ulp_distance(out, rgb).max() <= 4


def edge_frame():
    """32x32: two halves of different constant colour at depths 5 and 50, seeded noise of amplitude 0.05 on each."""
    r = np.random.default_rng(2024)
    right = np.zeros((32, 32), bool)
    right[:, 16:] = True
    base = np.where(right[..., None], np.float32([0.8, 0.3, 0.2]), np.float32([0.2, 0.5, 0.9]))
    rgb = (base + 0.05 * (2 * r.random((32, 32, 3)) - 1)).astype(np.float32)
    depth = np.where(right, 50, 5).astype(np.float32)
    return rgb, depth, np.full((32, 32), 4, np.uint32), right


def test_nothing_leaks_across_a_depth_step():
    rgb, depth, ns, right = edge_frame()
    for out in (denoise_ref(rgb, depth, ns, iterations=5), hip.denoise_host(rgb, depth, ns, iterations=5)):
        for half in (right, ~right):
            for ch in range(3):
                assert out[..., ch][half].min() >= rgb[..., ch][half].min() and out[..., ch][half].max() <= rgb[..., ch][half].max()
    out = hip.denoise_host(rgb, depth, ns, iterations=5)
    assert out[:, 16:, 0].std() < 0.5 * rgb[:, 16:, 0].std()   # (and each half was smoothed)


@pytest.fixture(scope="module")
def box_frames():
    """The oracle's Cornell box at 64x64: 4 spp and 256 spp."""
    from oracle import binding as oracle
    from qaray_amd.host import load_scene_blob
    blob = load_scene_blob("example_project12_box.xml", size=(64, 64))
    few = oracle.render(blob, (0, 0, 64, 64), 4)[:3]
    many = oracle.render(blob, (0, 0, 64, 64), 256)[0]
    return few, many


def test_a_denoised_preview_is_closer_to_the_converged_frame(box_frames):
    """Luma RMSE to the oracle's 256-spp frame: raw 4-spp frame 0.847, denoised (defaults) 0.519: ratio 0.613 on the host build.
    The filter must help at all, and the ratio must stay under the midpoint between that measurement and 1, 0.806."""
    (rgb, depth, ns), many = box_frames

    def rmse(x):
        return float(np.sqrt(np.mean((luma(x.astype(np.float64)) - luma(many.astype(np.float64))) ** 2)))
    raw, den = rmse(rgb), rmse(hip.denoise_host(rgb, depth, ns))
    print(f"luma RMSE raw {raw:.4f} denoised {den:.4f} ratio {den / raw:.4f}")
    assert den < raw
    assert den / raw < 0.5 * (0.613 + 1.0)


def _call(rgb, depth, ns, w, h, params, out):
    ptr = lambda a: None if a is None else a.ctypes.data
    return hip.lib().qa_test_denoise_host(ptr(rgb), ptr(depth), ptr(ns), w, h, None if params is None else C.byref(params), ptr(out))


def test_invalid_arguments_are_refused():
    rgb, depth, ns = random_frame(7, 5, 3)
    out = np.zeros_like(rgb)
    ok = hip.DenoiseParams.default()
    assert (ok.iterations, ok.sigma_color, ok.sigma_depth, ok.flags) == (5, 4.0, 1.0, 0)
    assert _call(rgb, depth, ns, 7, 5, ok, out) == 0
    with pytest.raises(hip.HipError) as e:
        hip.denoise_host(rgb, depth, ns, iterations=7)
    einval = e.value.code
    for bad in ((None, depth, ns, out), (rgb, None, ns, out), (rgb, depth, None, out), (rgb, depth, ns, None)):
        assert _call(*bad[:3], 7, 5, ok, bad[3]) == einval
    assert _call(rgb, depth, ns, 7, 5, None, out) == einval
    assert _call(rgb, depth, ns, 0, 5, ok, out) == einval and _call(rgb, depth, ns, 7, 0, ok, out) == einval
    assert _call(rgb, depth, ns, -7, 5, ok, out) == einval
    for field, values in (("iterations", (-1, 7)), ("sigma_color", (0.0, -1.0, np.nan, np.inf)), ("sigma_depth", (0.0, -2.0, np.nan, np.inf)),
                          ("flags", (1, 0x80000000))):
        for v in values:
            p = hip.DenoiseParams.default()
            setattr(p, field, v)
            assert _call(rgb, depth, ns, 7, 5, p, out) == einval, (field, v)
    assert hip.lib().qa_denoise_params_default(None) == einval
    for iterations in (0, 6):
        p = hip.DenoiseParams.default()
        p.iterations = iterations
        assert _call(rgb, depth, ns, 7, 5, p, out) == 0
