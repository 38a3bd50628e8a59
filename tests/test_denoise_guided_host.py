"""The guided form of the edge-avoiding filter (GUIDED FORM in qa_denoise_dev.h) on the CPU: qa_test_denoise_guided_host, the source
the device kernels are compiled from, against the float64 restatement of that section (tests/denoise_guided_util.py) and against
the rules the section states exactly.  tests/test_gpu_denoise_guided.py pins the device build to this one, bit for bit.

The section does not demodulate: dividing the colour by sample 0's albedo made 4-spp previews worse (DESIGN 4g has the figures), so
the albedo is an edge-stopping guide, as the normal is, and the properties checked here are those of that form."""
import ctypes as C

import numpy as np
import pytest

from denoise_guided_util import GUIDED_SIZES, HIT, MISS, VOID, bits, classes, denoise_guided_ref, guide_bits, guided_frame
from qaray_amd import hip


@pytest.mark.parametrize("w,h", GUIDED_SIZES)
def test_host_build_agrees_with_the_restatement(w, h):
    """Bound: 1e-4 of the frame's largest input component, as for the unguided filter (tests/test_denoise_host.py).  Measured: at
    most 1.5e-7 of it (40x33).  Between 30 % and 67 % of the pixels of these frames are reliable, so the guide terms run."""
    rgb, depth, ns, normal, albedo = guided_frame(w, h, 100 * w + h)
    cls = classes(rgb, depth, ns)
    live = cls != VOID
    if w * h > 1:
        reliable = guide_bits(cls, normal, albedo)[4]
        assert 0.25 < reliable.mean() < 0.75
    top = float(np.max(np.where(np.isfinite(rgb), rgb, 0)))
    for guides in ((normal, albedo), (normal, None), (None, albedo)):
        for iterations in (1, 3, 5, 6):
            got = hip.denoise_guided_host(rgb, depth, ns, *guides, iterations=iterations)
            want = denoise_guided_ref(rgb, depth, ns, *guides, iterations=iterations)
            assert np.array_equal(bits(got)[~live], bits(rgb)[~live])
            if live.any():
                dev = float(np.abs(got[live].astype(np.float64) - want[live]).max())
                print(f"{w}x{h} iterations {iterations}: deviation {dev / top:.3g} of the largest component")
                assert dev <= 1e-4 * top
    if w * h > 100:   # (and the guides did something)
        assert np.abs(hip.denoise_guided_host(rgb, depth, ns, normal, albedo)[live] - hip.denoise_host(rgb, depth, ns)[live]).max() > 0.05


def test_without_guides_it_is_the_unguided_filter_bit_for_bit():
    rgb, depth, ns, _, _ = guided_frame(33, 17, 5)
    for iterations in range(7):
        for sc, sd in ((4.0, 1.0), (1.5, 0.5)):
            assert np.array_equal(bits(hip.denoise_guided_host(rgb, depth, ns, iterations=iterations, sigma_color=sc, sigma_depth=sd, sigma_normal=0.3)),
                                  bits(hip.denoise_host(rgb, depth, ns, iterations=iterations, sigma_color=sc, sigma_depth=sd)))


def test_zero_iterations_return_the_input_bits_with_both_guides():
    rgb, depth, ns, normal, albedo = guided_frame(33, 17, 7)
    keep = [a.copy() for a in (rgb, depth, ns, normal, albedo)]
    assert np.array_equal(bits(hip.denoise_guided_host(rgb, depth, ns, normal, albedo, iterations=0)), bits(rgb))
    hip.denoise_guided_host(rgb, depth, ns, normal, albedo)
    for a, b in zip((rgb, depth, ns, normal, albedo), keep):   # the inputs are not modified
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint32), b.view(np.uint32))


def albedo_frame():
    """48x32, noiseless: rgb = albedo * 1.7 on a slanted plane; the albedo a checker of 8x8 squares, 0.45 / 0.70 grey: a step of 0.25,
    under the reliable bound 0.3, so every pixel is reliable and the albedo term runs on both sides of every edge."""
    h, w = 32, 48
    y, x = np.mgrid[0:h, 0:w]
    a = np.where(((x // 8 + y // 8) % 2 == 0)[..., None], np.float32(0.45), np.float32(0.70)) * np.ones(3, np.float32)
    rgb = (a * np.float32(1.7)).astype(np.float32)
    depth = (2 + 0.37 * x + 0.11 * y).astype(np.float32)
    return rgb, depth, np.full((h, w), 4, np.uint32), a.astype(np.float32)


def test_albedo_guide_keeps_a_painted_edge_that_the_unguided_filter_blurs():
    """Across an albedo step of 0.25 a reliable pixel's tap weighs exp(-0.25 / 0.02) = 3.7e-6 times its kernel weight at most, so
    no colour moves by more than 3.7e-6 * (the colour step 0.425) * (24 taps / the centre's 9/64 share), 3e-4 as a bound that needs
    no knowledge of the kernel; measured 7.2e-7.  The unguided filter moves the squares' edge pixels by up to 0.19, asserted 0.05 (the luma
    variance of their 3x3 window opens the colour weight): that is what the guide is for."""
    rgb, depth, ns, a = albedo_frame()
    assert guide_bits(classes(rgb, depth, ns), None, a)[4].all()
    guided = hip.denoise_guided_host(rgb, depth, ns, None, a)
    plain = hip.denoise_host(rgb, depth, ns)
    g, u = float(np.abs(guided - rgb).max()), float(np.abs(plain - rgb).max())
    print(f"largest change of a colour: guided {g:.3g}, unguided {u:.3g}")
    assert g < 3e-4
    assert u > 0.05


def normal_frame():
    """32x32: two halves at the same depth and slope (a fold seen head on), normals 90 degrees apart, different colours with seeded
    noise of amplitude 0.05 - the colour frame of test_denoise_host.edge_frame without its depth step."""
    r = np.random.default_rng(2024)
    right = np.zeros((32, 32), bool)
    right[:, 16:] = True
    base = np.where(right[..., None], np.float32([0.8, 0.3, 0.2]), np.float32([0.2, 0.5, 0.9]))
    rgb = (base + 0.05 * (2 * r.random((32, 32, 3)) - 1)).astype(np.float32)
    y, x = np.mgrid[0:32, 0:32]
    depth = (5 + 0.1 * np.abs(x - 15.5)).astype(np.float32)   # the same slope on both sides
    s = np.float32(np.sqrt(0.5))
    normal = np.where(right[..., None], np.float32([s, 0, s]), np.float32([-s, 0, s])).astype(np.float32)
    return rgb, depth, np.full((32, 32), 4, np.uint32), normal, right


def test_normal_guide_stops_the_leak_across_a_fold():
    """The leak bound of test_denoise_host.py for depth steps: every output stays in the closed range of its half's inputs, per
    channel.  The two columns next to the fold see the other normal in their 3x3 window, are not reliable and are filtered
    unguided by the specification - they are the pixels sample 0 describes from one side only - so the bound is asserted on the
    other 28 columns; without the guide those columns break it too."""
    rgb, depth, ns, normal, right = normal_frame()
    reliable = guide_bits(classes(rgb, depth, ns), normal, None)[4]
    inner = np.ones((32, 32), bool)
    inner[:, 15:17] = False
    assert np.array_equal(reliable, inner)

    def leaks(out):
        n = 0
        for half in (right & inner, ~right & inner):
            for ch in range(3):
                n += int(((out[..., ch][half] < rgb[..., ch][half].min()) | (out[..., ch][half] > rgb[..., ch][half].max())).sum())
        return n
    for out in (denoise_guided_ref(rgb, depth, ns, normal, None), hip.denoise_guided_host(rgb, depth, ns, normal, None)):
        assert leaks(out) == 0
    assert leaks(hip.denoise_host(rgb, depth, ns)) > 50
    out = hip.denoise_guided_host(rgb, depth, ns, normal, None)
    assert out[:, 17:, 0].std() < 0.5 * rgb[:, 17:, 0].std()   # (and each half was smoothed)


def test_invalid_guides_and_void_pixels_behave_as_specified():
    rgb, depth, ns, normal, albedo = guided_frame(33, 17, 11)
    cls = classes(rgb, depth, ns)
    void = cls == VOID
    out = hip.denoise_guided_host(rgb, depth, ns, normal, albedo)
    assert void.sum() > 5 and np.array_equal(bits(out)[void], bits(rgb)[void]) and np.isfinite(out[~void]).all()
    # a normal that is 0 or not finite takes no normal term: any other invalid value in its place gives the same bits
    n32 = normal.copy()
    bad = (cls == HIT) & ~guide_bits(cls, normal, None)[1]
    assert bad.sum() > 5
    n32[bad] = np.float32([np.inf, 0, np.nan])
    assert np.array_equal(bits(hip.denoise_guided_host(rgb, depth, ns, n32, albedo)), bits(out))
    n32[bad] = 0
    assert np.array_equal(bits(hip.denoise_guided_host(rgb, depth, ns, n32, albedo)), bits(out))
    # so does an albedo with a component that is not finite; a component 0 is an albedo like any other
    a32 = albedo.copy()
    bad = ~void & ~guide_bits(cls, None, albedo)[3]
    assert bad.sum() > 5
    a32[bad] = np.float32([np.nan, 0.5, -np.inf])
    assert np.array_equal(bits(hip.denoise_guided_host(rgb, depth, ns, normal, a32)), bits(out))
    a32 = albedo.copy()
    zero = ~void & (albedo[..., 0] == 0)
    assert zero.any()
    a32[zero, 0] = np.float32(0.9)
    assert not np.array_equal(bits(hip.denoise_guided_host(rgb, depth, ns, normal, a32)), bits(out))
    # the guides of void pixels are never looked at, and a miss pixel's normal is not
    n32, a32 = normal.copy(), albedo.copy()
    n32[void | (depth == MISS)] = np.float32([1, 2, 3])
    a32[void] = np.float32(7)
    assert np.array_equal(bits(hip.denoise_guided_host(rgb, depth, ns, n32, a32)), bits(out))


def _call(rgb, depth, ns, normal, albedo, w, h, params, out):
    ptr = lambda a: None if a is None else a.ctypes.data
    return hip.lib().qa_test_denoise_guided_host(ptr(rgb), ptr(depth), ptr(ns), ptr(normal), ptr(albedo), w, h, None if params is None else C.byref(params),
                                                 ptr(out))


def test_invalid_arguments_are_refused():
    rgb, depth, ns, normal, albedo = guided_frame(7, 5, 3)
    out = np.zeros_like(rgb)
    ok = hip.DenoiseGuidedParams.default()
    assert (ok.iterations, ok.sigma_color, ok.sigma_depth, ok.flags) == (5, 4.0, 1.0, 3) and abs(ok.sigma_normal - 0.1) < 1e-8
    assert _call(rgb, depth, ns, normal, albedo, 7, 5, ok, out) == 0
    with pytest.raises(hip.HipError) as e:
        hip.denoise_guided_host(rgb, depth, ns, normal, albedo, iterations=7)
    einval = e.value.code
    for k in range(3):
        args = [rgb, depth, ns]
        args[k] = None
        assert _call(*args, normal, albedo, 7, 5, ok, out) == einval
    assert _call(rgb, depth, ns, normal, albedo, 7, 5, ok, None) == einval
    assert _call(rgb, depth, ns, normal, albedo, 7, 5, None, out) == einval
    assert _call(rgb, depth, ns, normal, albedo, 0, 5, ok, out) == einval and _call(rgb, depth, ns, normal, albedo, 7, -5, ok, out) == einval
    # a plane is given if and only if its bit is set
    assert _call(rgb, depth, ns, None, albedo, 7, 5, ok, out) == einval and _call(rgb, depth, ns, normal, None, 7, 5, ok, out) == einval
    for flags, n, a in ((0, normal, None), (0, None, albedo), (1, None, None), (1, normal, albedo), (2, normal, albedo), (2, None, None)):
        p = hip.DenoiseGuidedParams.default()
        p.flags = flags
        assert _call(rgb, depth, ns, n, a, 7, 5, p, out) == einval, flags
    for flags, n, a in ((0, None, None), (1, normal, None), (2, None, albedo)):
        p = hip.DenoiseGuidedParams.default()
        p.flags = flags
        assert _call(rgb, depth, ns, n, a, 7, 5, p, out) == 0, flags
    for field, values in (("iterations", (-1, 7)), ("sigma_color", (0.0, -1.0, np.nan, np.inf)), ("sigma_depth", (0.0, -2.0, np.nan, np.inf)),
                          ("sigma_normal", (0.0, -0.1, np.nan, np.inf)), ("flags", (4, 7, 0x80000003))):
        for v in values:
            p = hip.DenoiseGuidedParams.default()
            setattr(p, field, v)
            assert _call(rgb, depth, ns, normal, albedo, 7, 5, p, out) == einval, (field, v)
    assert hip.lib().qa_denoise_guided_params_default(None) == einval
