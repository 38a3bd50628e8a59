"""The variance form of the edge-avoiding filter (VARIANCE FORM in qa_denoise_dev.h) on the CPU: qa_test_denoise_variance_host, the
source the device kernels are compiled from, against the guided form it extends, against the float64 restatement of that section
(tests/denoise_variance_util.py), against the rules the section states exactly and - for the one claim about quality - against the
oracle's converged frames.  tests/test_gpu_denoise_variance.py pins the device build to this one, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import denoise_variance_util as vu
from denoise_guided_util import GUIDED_SIZES, guided_frame
from denoise_variance_util import HIT, MISS, VOID, bits, classes, denoise_variance_ref, luma, variance_frame
from qaray_amd import hip


@pytest.mark.parametrize("w,h", GUIDED_SIZES)
def test_without_the_plane_and_with_a_plane_of_minus_one_it_is_the_guided_form_bit_for_bit(w, h):
    rgb, depth, ns, normal, albedo = guided_frame(w, h, 100 * w + h)
    none = np.full((h, w), -1, np.float32)
    for guides in ((normal, albedo), (normal, None), (None, albedo), (None, None)):
        for iterations in (0, 1, 2, 5):
            want = bits(hip.denoise_guided_host(rgb, depth, ns, *guides, iterations=iterations))
            assert np.array_equal(bits(hip.denoise_variance_host(rgb, depth, ns, *guides, None, iterations=iterations, variance_scale=9.0)), want)
            assert np.array_equal(bits(hip.denoise_variance_host(rgb, depth, ns, *guides, none, iterations=iterations, variance_scale=9.0)), want)
    assert np.array_equal(bits(hip.denoise_variance_host(rgb, depth, ns, None, None, None)), bits(hip.denoise_host(rgb, depth, ns)))


@pytest.mark.parametrize("w,h", vu.VARIANCE_SIZES + ((40, 33),))
def test_host_build_agrees_with_the_restatement(w, h):
    """Measured: at most 1.34e-5 of the frame's largest input component (33x35; 1.5e-7 and less at the other sizes - a plane value of 0
    leaves den_l at its floor of 1e-4, where a rounding of the luma weighs most).  Asserted: 4 x that, 5.4e-5, inside the 1e-4 that
    bounds the two forms below it."""
    rgb, depth, ns, normal, albedo, var = variance_frame(w, h, 100 * w + h)
    cls = classes(rgb, depth, ns)
    live = cls != VOID
    top = float(np.max(np.where(np.isfinite(rgb), rgb, 0)))
    worst = 0.0
    for guides in ((normal, albedo), (None, None), (None, albedo)):
        for iterations, scale in ((1, 4.0), (3, 0.5), (5, 4.0), (6, 16.0)):
            got = hip.denoise_variance_host(rgb, depth, ns, *guides, var, iterations=iterations, variance_scale=scale)
            want = denoise_variance_ref(rgb, depth, ns, *guides, var, iterations=iterations, variance_scale=scale)
            assert np.array_equal(bits(got)[~live], bits(rgb)[~live])
            if live.any():
                dev = float(np.abs(got[live].astype(np.float64) - want[live]).max())
                worst = max(worst, dev / top)
                assert dev <= vu.RESTATEMENT_BOUND * top
    print(f"{w}x{h}: largest deviation {worst:.3g} of the largest component")
    if w * h > 100:   # (and the plane did something)
        assert np.abs(hip.denoise_variance_host(rgb, depth, ns, normal, albedo, var)[live] - hip.denoise_guided_host(rgb, depth, ns, normal, albedo)[live]).max() > 0.01


def flat_frame(w=9, h=7, seed=3):
    r = np.random.default_rng(seed)
    rgb = (0.5 + r.random((h, w, 3))).astype(np.float32)
    y, x = np.mgrid[0:h, 0:w]
    return rgb, (4 + 0.1 * x + 0.05 * y).astype(np.float32), np.full((h, w), 4, np.uint32)


def pass0_var(rgb, depth, ns, variance, scale):
    """The restatement's pass 0 -> (var, the spatial var, trusted), float64."""
    cls = classes(rgb, depth, ns)
    return vu.pass0_variance(cls, luma(np.where((cls != VOID)[..., None], rgb.astype(np.float64), 0.0)), variance, scale)


def test_a_lone_trusted_pixel_takes_scale_times_its_value_exactly():
    """A trusted pixel with no other trusted member in its window has var = variance_scale * t_p: the output is that of a plane in
    which the window's other members hold t_p too (their own var is not p's business: they stay untrusted here, so both runs differ
    only in p's var, and equal outputs at p's taps say the var was the same).  Checked through the restatement to 1e-4 and, exactly,
    by scaling: (scale, t) and (2 scale, t / 2) give the same bits."""
    rgb, depth, ns = flat_frame()
    var = np.full(depth.shape, -1, np.float32)
    var[3, 4] = np.float32(0.0371)
    a = hip.denoise_variance_host(rgb, depth, ns, None, None, var, iterations=1, variance_scale=4.0)
    half = var.copy()
    half[3, 4] = var[3, 4] / 2
    b = hip.denoise_variance_host(rgb, depth, ns, None, None, half, iterations=1, variance_scale=8.0)
    assert np.array_equal(bits(a), bits(b))
    v, spatial, tr = pass0_var(rgb, depth, ns, var, 4.0)
    assert tr.sum() == 1 and v[3, 4] == 4.0 * float(var[3, 4]) and np.array_equal(v[~tr], spatial[~tr])
    want = denoise_variance_ref(rgb, depth, ns, None, None, var, iterations=1, variance_scale=4.0)
    assert np.abs(a - want).max() <= 1e-4 * float(rgb.max())
    plain = hip.denoise_guided_host(rgb, depth, ns, iterations=1)
    assert not np.array_equal(bits(a[3, 4]), bits(plain[3, 4]))
    # one iteration at step 1 reaches two pixels: the pixels further from (3, 4) have the guided form's bits
    far = np.ones(depth.shape, bool)
    far[1:6, 2:7] = False
    assert np.array_equal(bits(a[far]), bits(plain[far]))


def test_an_untrusted_pixel_keeps_the_spatial_value_bit_for_bit():
    """Every pixel but a block is untrusted: after one iteration the pixels whose 5x5 taps hold no trusted pixel equal the guided form
    bit for bit - they and all their taps kept the spatial var - and so does every untrusted pixel's own var, which the restatement
    shows."""
    rgb, depth, ns = flat_frame(21, 17, 5)
    var = np.full(depth.shape, -1, np.float32)
    var[6:9, 8:12] = np.float32(0.02)
    a = hip.denoise_variance_host(rgb, depth, ns, None, None, var, iterations=1)
    plain = hip.denoise_guided_host(rgb, depth, ns, iterations=1)
    far = np.ones(depth.shape, bool)
    far[4:11, 6:14] = False
    assert np.array_equal(bits(a[far]), bits(plain[far])) and not np.array_equal(bits(a[~far]), bits(plain[~far]))
    v, spatial, tr = pass0_var(rgb, depth, ns, var, 4.0)
    assert np.array_equal(v[~tr], spatial[~tr]) and np.allclose(v[tr], 0.08)


@pytest.mark.parametrize("bad", (-1.0, -1e-30, np.nan, np.inf, -np.inf))
def test_a_negative_nan_or_infinite_plane_value_is_none(bad):
    rgb, depth, ns, normal, albedo, var = variance_frame(33, 17, 11)
    cls = classes(rgb, depth, ns)
    none = ~vu.trusted_plane(cls, var)
    other = var.copy()
    other[none] = np.float32(bad)
    assert none.sum() > 100
    assert np.array_equal(bits(hip.denoise_variance_host(rgb, depth, ns, normal, albedo, other)), bits(hip.denoise_variance_host(rgb, depth, ns, normal, albedo, var)))


def test_void_miss_and_mixed_windows():
    rgb, depth, ns = flat_frame(21, 17, 7)
    depth[:, 12:] = MISS                       # a border between the classes
    ns[5, 5] = 0
    rgb[9, 9, 1] = np.nan
    var = np.full(depth.shape, np.float32(0.01))
    var[:, 12:] = np.float32(0.5)              # the misses' values must not enter a hit pixel's window, nor the other way
    keep = [a.copy() for a in (rgb, depth, ns, var)]
    out = hip.denoise_variance_host(rgb, depth, ns, None, None, var, variance_scale=1.0)
    for a, b in zip((rgb, depth, ns, var), keep):   # the inputs are not modified
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint32), b.view(np.uint32))
    cls = classes(rgb, depth, ns)
    void = cls == VOID
    assert void.sum() == 2 and np.array_equal(bits(out)[void], bits(rgb)[void]) and np.isfinite(out[~void]).all()
    v, _, tr = pass0_var(rgb, depth, ns, var, 1.0)
    assert np.allclose(v[(cls == HIT)], 0.01) and np.allclose(v[cls == 1], 0.5) and tr.sum() == 21 * 17 - 2
    # a void pixel's plane value is never looked at, nor its colour
    var2, rgb2 = var.copy(), rgb.copy()
    var2[void] = np.float32(77)
    rgb2[5, 5] = 1e6
    assert np.array_equal(bits(hip.denoise_variance_host(rgb2, depth, ns, None, None, var2, variance_scale=1.0))[~void], bits(out)[~void])
    want = denoise_variance_ref(rgb, depth, ns, None, None, var, variance_scale=1.0)
    assert np.abs(out[~void] - want[~void]).max() <= 1e-4 * 1.5
    # each class is filtered among its own: changing the other side's plane moves nothing on this side
    var3 = var.copy()
    var3[:, 12:] = np.float32(0.001)
    out3 = hip.denoise_variance_host(rgb, depth, ns, None, None, var3, variance_scale=1.0)
    hitp = cls == HIT
    assert np.array_equal(bits(out3)[hitp], bits(out)[hitp]) and not np.array_equal(bits(out3)[cls == 1], bits(out)[cls == 1])


def test_zero_iterations_return_the_input_bits():
    rgb, depth, ns, normal, albedo, var = variance_frame(33, 17, 7)
    assert np.array_equal(bits(hip.denoise_variance_host(rgb, depth, ns, normal, albedo, var, iterations=0)), bits(rgb))
    assert np.array_equal(bits(hip.denoise_variance_host(rgb, depth, ns, None, None, var, iterations=0)), bits(rgb))


# ---- quality: the oracle's frames, accumulated ------------------------------------------------------------------------

def quality(which, scale=None):
    p = vu.oracle_preview(which)
    ns = p["ns"].astype(np.uint32)
    guided = hip.denoise_guided_host(p["acc"], p["depth"], ns, None, p["albedo"])
    kw = {} if scale is None else dict(variance_scale=scale)
    with_var = hip.denoise_variance_host(p["acc"], p["depth"], ns, None, p["albedo"], p["variance"], **kw)
    return dict(raw=vu.luma_rmse(p["raw"], p["truth"]), acc=vu.luma_rmse(p["acc"], p["truth"]), i=vu.luma_rmse(guided, p["truth"]),
                ii=vu.luma_rmse(with_var, p["truth"]))


def test_the_variance_plane_makes_an_accumulated_preview_closer_to_the_converged_frame():
    """Eight 4-spp oracle frames of different seeds, still camera, accumulated with the moments; the accumulated frame filtered (i) by
    the guided form and (ii) by the variance form at its defaults, with the albedo plane (the CPU has no normal plane).  Luma RMSE to
    the 256-spp frame, host build:
      custom_textures.xml 64x64: raw 0.0324, accumulated 0.0276, (i) 0.0302, (ii) 0.0265: (ii) / (i) = 0.877
      Cornell box 64x64:         raw 0.8860, accumulated 0.5476, (i) 0.5162, (ii) 0.4955: (ii) / (i) = 0.960
    On the textured scene the guided form takes converged texture for noise and lands above the unfiltered accumulation; with the
    temporal variance it lands below it.  DESIGN.md 4k has the sweep over variance_scale behind the default."""
    t, b = quality("textures"), quality("box")
    for name, q in (("custom_textures.xml", t), ("Cornell box", b)):
        print(f"{name}: raw {q['raw']:.4f}, accumulated {q['acc']:.4f}, guided (i) {q['i']:.4f}, variance form (ii) {q['ii']:.4f}, (ii) / (i) {q['ii'] / q['i']:.4f}")
    assert t["ii"] < t["i"]
    assert b["ii"] <= 1.02 * b["i"]
    assert t["ii"] < t["raw"] and b["ii"] < b["raw"]


def test_the_default_scale_is_the_sweeps_choice():
    """The rule of DESIGN.md 4k: among the scales with (ii) <= 1.02 x (i) on the box, the lowest (ii) / (i) on the textured scene."""
    rows = {s: (quality("textures", s), quality("box", s)) for s in vu.VARIANCE_SCALES}
    for s, (t, b) in rows.items():
        print(f"variance_scale {s}: textures (ii) / (i) {t['ii'] / t['i']:.4f}, box (ii) / (i) {b['ii'] / b['i']:.4f}")
    allowed = [s for s, (t, b) in rows.items() if b["ii"] <= 1.02 * b["i"]]
    best = min(allowed, key=lambda s: rows[s][0]["ii"] / rows[s][0]["i"])
    assert best == hip.DenoiseVarianceParams.default().variance_scale


# ---- refusals -----------------------------------------------------------------------------------------------------------------------

def _call(rgb, depth, ns, normal, albedo, var, w, h, params, out):
    ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    return hip.lib().qa_test_denoise_variance_host(ptr(rgb), ptr(depth), ptr(ns), ptr(normal), ptr(albedo), ptr(var), w, h,
                                                   None if params is None else C.byref(params), ptr(out))


def test_invalid_arguments_are_refused():
    rgb, depth, ns, normal, albedo, var = variance_frame(7, 5, 3)
    out = np.zeros_like(rgb)
    ok = hip.DenoiseVarianceParams.default()
    assert (ok.iterations, ok.sigma_color, ok.sigma_depth, ok.flags, ok.variance_scale) == (5, 4.0, 1.0, 7, 4.0) and abs(ok.sigma_normal - 0.1) < 1e-8
    assert hip.QA_DENOISE_GUIDE_VARIANCE == 4 and C.sizeof(ok) == 24
    assert _call(rgb, depth, ns, normal, albedo, var, 7, 5, ok, out) == 0
    with pytest.raises(hip.HipError) as e:
        hip.denoise_variance_host(rgb, depth, ns, normal, albedo, var, iterations=7)
    einval = e.value.code
    for k in range(3):
        args = [rgb, depth, ns]
        args[k] = None
        assert _call(*args, normal, albedo, var, 7, 5, ok, out) == einval
    assert _call(rgb, depth, ns, normal, albedo, var, 7, 5, ok, None) == einval
    assert _call(rgb, depth, ns, normal, albedo, var, 7, 5, None, out) == einval
    assert _call(rgb, depth, ns, normal, albedo, var, 0, 5, ok, out) == einval and _call(rgb, depth, ns, normal, albedo, var, 7, -5, ok, out) == einval
    # a plane is given if and only if its bit is set
    for flags, n, a, v in ((7, normal, albedo, None), (3, normal, albedo, var), (4, None, None, None), (0, None, None, var), (6, normal, albedo, var),
                           (5, None, albedo, var)):
        p = hip.DenoiseVarianceParams.default()
        p.flags = flags
        assert _call(rgb, depth, ns, n, a, v, 7, 5, p, out) == einval, flags
    for flags, n, a, v in ((0, None, None, None), (4, None, None, var), (5, normal, None, var), (6, None, albedo, var), (3, normal, albedo, None)):
        p = hip.DenoiseVarianceParams.default()
        p.flags = flags
        assert _call(rgb, depth, ns, n, a, v, 7, 5, p, out) == 0, flags
    for field, values in (("iterations", (-1, 7)), ("sigma_color", (0.0, -1.0, np.nan, np.inf)), ("sigma_depth", (0.0, -2.0, np.nan, np.inf)),
                          ("sigma_normal", (0.0, -0.1, np.nan, np.inf)), ("variance_scale", (0.0, -4.0, np.nan, np.inf)), ("flags", (8, 15, 0x80000007))):
        for v in values:
            p = hip.DenoiseVarianceParams.default()
            setattr(p, field, v)
            assert _call(rgb, depth, ns, normal, albedo, var, 7, 5, p, out) == einval, (field, v)
    assert hip.lib().qa_denoise_variance_params_default(None) == einval
