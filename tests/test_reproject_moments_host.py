"""Reprojection with luminance moments and a shortened length on the CPU (qa_test_reproject_moments_host:
qaray_amd/csrc/hip/qa_reproject_moments_dev.h built for the host) against the form it extends, against a float64 numpy restatement
of the header's specification (tests/reproject_moments_util.py) and against the statistics the variance is meant to estimate.  No
GPU: tests/test_gpu_reproject_moments.py pins the kernel to this build bit for bit."""
import ctypes as C

import numpy as np
import pytest

import reproject_moments_util as xu
import reproject_motion_util as mu
import reproject_util as ru
from qaray_amd import hip
from reproject_moments_util import call_moments, moments_inputs, restate_moments
from reproject_motion_util import call_motion, motion_inputs
from reproject_util import H, MISS, W, bits, call, inputs

QA_EINVAL = -1
UNDECIDED_CAP = 0.02


def same_bits(got, want, what, names=("out", "length", "moments", "variance")):
    for g, w, name in zip(got, want, names):
        bad = np.argwhere(bits(g) != bits(w))
        assert bad.size == 0, (what, name, len(bad), bad[:5])


def deviation(out, ref, mask):
    return float(np.abs(out[mask] - ref[mask]).max() / max(np.abs(ref[mask]).max(), 1e-30)) if mask.any() else 0.0


# ---- 1. new flags off: the motion form's bits ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("still", (False, True))
@pytest.mark.parametrize("size,origin", (((W, H), (0, 0)), ((62, 42), (5, 3))))
def test_new_flags_off_give_the_motion_forms_bits(size, origin, still):
    a = inputs(size[0], size[1], origin, seed=2, still=still)
    for ids in (True, False):
        got = call(hip.reproject_moments_host, a, ids)
        assert got[2] is None and got[3] is None
        same_bits(got[:2], call(hip.reproject_motion_host, a, ids), (ids,))
        kw = dict(max_history=8, depth_tolerance=0.2, clamp=True, clamp_radius=2, clamp_gamma=0.5)
        same_bits(call(hip.reproject_moments_host, a, ids, **kw)[:2], call(hip.reproject_motion_host, a, ids, **kw), (ids, "parameters"))
    m = motion_inputs(size[0], size[1], origin, seed=3, still=still)
    same_bits(call_moments(hip.reproject_moments_host, m, clamp=True)[:2], call_motion(hip.reproject_motion_host, m, clamp=True), "motion and clamp")
    # the two parameters of the new flags are not read without them, and planes given without MOMENTS are not written
    om, ov = np.full((size[1], size[0], 2), 7, np.float32), np.full((size[1], size[0]), 7, np.float32)
    got = call_moments(hip.reproject_moments_host, m, clamp=True, min_frames=float("nan"), shorten_rate=-1.0, out_moments=om, out_variance=ov)
    same_bits(got[:2], call_motion(hip.reproject_motion_host, m, clamp=True), "unread parameters")
    assert (om == 7).all() and (ov == 7).all()


@pytest.mark.parametrize("name,a", ru.edge_cases(), ids=[n for n, _ in ru.edge_cases()])
def test_new_flags_off_give_the_motion_forms_bits_on_the_edge_cases(name, a):
    for ids in (True, False):
        for kw in ({}, dict(clamp=True)):
            same_bits(call(hip.reproject_moments_host, a, ids, **kw)[:2], call(hip.reproject_motion_host, a, ids, **kw), (name, ids, kw))


@pytest.mark.parametrize("name,a", ru.edge_cases(), ids=[n for n, _ in ru.edge_cases()])
def test_the_edge_cases_with_all_new_flags_make_nothing_that_is_not_a_number(name, a):
    h, w = a["cur"][1].shape
    r = np.random.default_rng(5)
    mom = r.random((h, w, 2), dtype=np.float32)
    out, length, om, ov = call(hip.reproject_moments_host, a, True, hist_moments=mom, clamp=True, moments=True, shorten=True)
    void = (a["cur"][2] == 0) | ~np.isfinite(a["cur"][0]).all(-1) | ~np.isfinite(a["cur"][1])
    assert np.isfinite(out[~void]).all() and np.isfinite(length).all() and np.isfinite(om).all() and np.isfinite(ov).all()
    assert (om[void] == 0).all() and (ov[void] == -1).all() and (length[void] == 0).all()
    assert ((ov == -1) | (ov >= 0)).all()


def test_defaults():
    p = hip.ReprojectMomentsParams.default()
    assert (p.depth_tolerance, p.max_history, p.flags) == (np.float32(0.05), 64.0, 0)
    assert (p.clamp_radius, p.clamp_gamma, p.min_frames) == (1, 1.0, 4.0)
    assert p.shorten_rate == 4.0    # the sweep behind it
    assert (hip.QA_REPROJECT_MOMENTS, hip.QA_REPROJECT_SHORTEN) == (4, 8) and C.sizeof(p) == 28


# ---- 2. against the restatement ----------------------------------------------------------------------------------------------------

FLAG_SETS = {"moments": dict(moments=True), "clamp+shorten": dict(clamp=True, shorten=True, clamp_radius=2),
             "all four": dict(clamp=True, shorten=True, moments=True, clamp_radius=2)}


@pytest.mark.parametrize("still", (False, True), ids=("moving camera", "still camera"))
@pytest.mark.parametrize("flags", list(FLAG_SETS))
def test_host_equals_the_restatement(flags, still):
    # (min_frames 3.1: the still camera keeps the integer lengths 5 .. 23 of the inputs, which a threshold of 12 would meet exactly)
    kw = dict(FLAG_SETS[flags], min_frames=3.1, shorten_rate=0.5)
    a = moments_inputs(seed=1, still=still)
    use_motion = flags == "all four"
    before = [np.array(x, copy=True) for x in (*a["cur"], *a["hist"], a["ids"], a["hist_ids"], a["hist_moments"])]
    out, length, om, ov = call_moments(hip.reproject_moments_host, a, motion=use_motion, **kw)
    for x, y in zip(before, (*a["cur"], *a["hist"], a["ids"], a["hist_ids"], a["hist_moments"])):
        assert np.array_equal(bits(x), bits(y))
    R = call_moments(restate_moments, a, motion=use_motion, **kw)
    assert R["undecided"].mean() <= UNDECIDED_CAP, R["undecided"].mean()
    dec = ~R["undecided"] & ~R["void"]
    dev = dict(colour=deviation(out, R["out"], dec), length=deviation(length, R["length"], dec))
    if "shorten" in kw:
        assert (R["b"] > 0.1).sum() > 1000    # (a history inside its box, b == 0: section 4 below)
    if "moments" in kw:
        assert R["trusted"].sum() > 300 and (R["has_moments"] & ~R["trusted"]).sum() > 100 and (R["has"] & ~R["has_moments"]).sum() >= 2
        dev["moments"] = deviation(om, R["moments"], dec)
        both = dec & R["trusted"]
        assert np.array_equal((ov >= 0)[dec], R["trusted"][dec])
        assert (ov[dec & ~R["trusted"]] == -1).all()
        dev["variance"] = deviation(ov, R["variance"], both)
    print(f"{flags}, still {still}: " + ", ".join(f"{k} {v:.3g}" for k, v in dev.items()) + f"; undecided {R['undecided'].mean():.4f}")
    assert dev["colour"] <= xu.COLOUR_BOUND and dev["length"] <= xu.LENGTH_BOUND
    assert dev.get("moments", 0.0) <= xu.MOMENTS_BOUND and dev.get("variance", 0.0) <= xu.VARIANCE_BOUND
    assert np.array_equal((length > a["cur"][2])[dec], R["has"][dec])
    none = dec & ~R["has"]
    assert np.array_equal(bits(out[none]), bits(a["cur"][0][none]))


# ---- 3. against the truth ----------------------------------------------------------------------------------------------------------

def still_flat(w=64, h=64, ns=4):
    c = ru.cam0()
    depth = np.full((h, w), 5, np.float32)
    return c, depth, np.full((h, w), ns, np.uint32)


def accumulate(frames, depth, ns, cam, **kw):
    """The frames pushed one after another through the host form with MOMENTS, a still camera -> the last call's four planes."""
    h, w = depth.shape
    hist = (np.zeros((h, w, 3), np.float32), depth, np.zeros((h, w), np.float32))
    mom = None
    res = None
    for f in frames:
        res = hip.reproject_moments_host((f, depth, ns), hist, cam, cam, hist_moments=mom, moments=True, **kw)
        hist, mom = (res[0], depth, res[1]), res[2]
    return res


def grey_frames(count, mu_, sigma, seed, w=64, h=64):
    g = np.random.default_rng(seed).standard_normal((count, h, w))
    return [np.repeat((mu_ + sigma * x)[..., None], 3, axis=-1).astype(np.float32) for x in g]


def test_the_variance_estimates_the_spread_of_the_frames():
    """Bound (derived, not measured): with equal weights o1 and o2 are the sample mean and the mean square of the N lumas, so
    v = o2 - o1^2 is the biased sample variance, whose expectation is sigma^2 (N - 1) / N.  The mean of v over 4 096 independent
    pixels has the relative standard deviation sqrt(2 / (N - 1)) / 64 = 0.6 % at N = 16: 5 % is eight of them."""
    N, mean, sigma = 16, 1.0, 0.2
    cam, depth, ns = still_flat()
    frames = grey_frames(N, mean, sigma, seed=2024)
    out, length, om, ov = accumulate(frames, depth, ns, cam, max_history=1e6)
    assert (ov >= 0).all() and np.array_equal(length, np.full_like(length, 4.0 * N))
    k = 1.0 / N
    got = float(np.mean(ov.astype(np.float64) / k))
    want = sigma * sigma * (N - 1) / N
    print(f"mean of out_variance / k: {got:.6g}, sigma^2 (N - 1) / N: {want:.6g}, ratio {got / want:.4f}")
    assert abs(got / want - 1) <= 0.05
    lum = np.mean([xu.luma64(f) for f in frames], axis=0)
    assert np.abs(om[..., 0] - lum).max() <= 1e-5
    # and out_variance is the variance of the accumulated colour's luma: over the pixels, the accumulated luma's spread about mean
    acc_var = float(np.var(xu.luma64(out)))
    print(f"variance of the accumulated luma over the pixels {acc_var:.4g}, mean out_variance {float(ov.mean()):.4g}")
    assert abs(float(ov.mean()) / acc_var - 1) <= 0.15    # (N - 1) / N = 6 % low, and 0.6 % + 2.2 % (the spread of acc_var) of noise


def test_the_trust_threshold():
    cam, depth, ns = still_flat(9, 7)
    frames = grey_frames(4, 1.0, 0.2, seed=3, w=9, h=7)
    assert (accumulate(frames[:3], depth, ns, cam)[3] == -1).all()
    assert (accumulate(frames, depth, ns, cam)[3] >= 0).all()
    assert (accumulate(frames, depth, ns, cam, min_frames=4.5)[3] == -1).all()
    assert (accumulate(frames[:1], depth, ns, cam, min_frames=1.0)[3] == -1).all()     # no moment history on the first frame
    assert (accumulate(frames[:2], depth, ns, cam, min_frames=1.0)[3] >= 0).all()
    # in samples, not frames: history of 2 samples a frame is still short of 4 x 4 after five frames, and there after seven
    two = np.full_like(ns, 2)
    hist = accumulate(frames * 2, depth, two, cam)      # 8 frames of 2: length 16
    assert (hist[1] == 16).all()
    five = accumulate(frames + frames[:1], depth, two, cam)    # length 10
    res = hip.reproject_moments_host((frames[0], depth, ns), (five[0], depth, five[1]), cam, cam, hist_moments=five[2], moments=True)
    assert (res[1] == 14).all() and (res[3] == -1).all()
    res = hip.reproject_moments_host((frames[0], depth, ns), (hist[0], depth, hist[1]), cam, cam, hist_moments=hist[2], moments=True)
    assert (res[1] == 20).all() and (res[3] >= 0).all()


def test_without_a_moments_plane_nobody_has_moment_history():
    a = moments_inputs(seed=4)
    out, length, om, ov = call_moments(hip.reproject_moments_host, dict(a, hist_moments=None), moments=True)
    same_bits((out, length), call_motion(hip.reproject_motion_host, a), "colour and length")
    void = length == 0
    l = xu.luma64(a["cur"][0])
    with np.errstate(invalid="ignore"):
        assert np.abs(om[~void, 0] - l[~void]).max() <= 1e-6 and np.abs(om[~void, 1] - (l * l)[~void]).max() <= 1e-6
    assert (om[void] == 0).all() and (ov == -1).all()


def test_a_moment_that_is_not_finite_in_a_counting_tap():
    cam, depth, ns = still_flat(9, 7)
    frames = grey_frames(5, 1.0, 0.2, seed=6, w=9, h=7)
    h = accumulate(frames[:4], depth, ns, cam)
    mom = h[2].copy()
    mom[3, 4, 1] = np.nan
    mom[5, 2, 0] = np.inf
    res = hip.reproject_moments_host((frames[4], depth, ns), (h[0], depth, h[1]), cam, cam, hist_moments=mom, moments=True)
    ref = hip.reproject_moments_host((frames[4], depth, ns), (h[0], depth, h[1]), cam, cam, hist_moments=h[2], moments=True)
    same_bits(res[:2], ref[:2], "colour history kept")
    bad = np.zeros((7, 9), bool)
    bad[3, 4] = bad[5, 2] = True
    l = xu.luma64(frames[4]).astype(np.float32)
    assert (res[3][bad] == -1).all() and np.array_equal(bits(res[2][bad][:, 0]), bits(l[bad])) and np.array_equal(bits(res[2][bad][:, 1]), bits(l[bad] * l[bad]))
    same_bits((res[2][~bad], res[3][~bad]), (ref[2][~bad], ref[3][~bad]), "the others", ("moments", "variance"))
    assert (ref[3] >= 0).all()


# ---- 4. the shortened length -------------------------------------------------------------------------------------------------------

def test_a_history_inside_the_box_keeps_the_flag_off_bits():
    a = mu_flat(seed=1)
    _, mean, _, _ = mu.window_stats(*a["cur"], 1)
    a["hist"] = (mean.astype(np.float32), *a["hist"][1:])
    mom = np.random.default_rng(1).random((*mean.shape[:2], 2), dtype=np.float32)
    kw = dict(motion=False, ids=False, clamp=True, moments=True)
    on = call_moments(hip.reproject_moments_host, dict(a, hist_moments=mom), shorten=True, shorten_rate=4.0, **kw)
    off = call_moments(hip.reproject_moments_host, dict(a, hist_moments=mom), shorten=False, **kw)
    same_bits(on, off, "inside the box")
    same_bits(on[:2], call_motion(hip.reproject_motion_host, a, motion=False, ids=False, clamp=True), "the motion form")


def mu_flat(seed=0, w=23, h=19):
    """tests/test_reproject_motion_host.py's flat_inputs: a still camera over constant depth, every pixel its own single tap."""
    r = np.random.default_rng(seed)
    c = ru.cam0()
    return dict(c0=c, c1=c, cur=(r.random((h, w, 3), dtype=np.float32) + np.float32(0.5), np.full((h, w), 5, np.float32), np.full((h, w), 4, np.uint32)),
                hist=(np.zeros((h, w, 3), np.float32), np.full((h, w), 5, np.float32), np.full((h, w), 60, np.float32)), origin=(0, 0), ids=None,
                hist_ids=None, motion=None)


@pytest.mark.parametrize("gamma", (0.0, 1.0))
def test_a_far_history_loses_its_length(gamma):
    a = mu_flat(seed=2)
    a["cur"][0][...] = (a["cur"][0] - np.float32(1.0)) * np.float32(1e-3) + np.float32(1.0)    # a quiet window: sigma of about 3e-4
    a["hist"] = (np.full_like(a["cur"][0], 100 * a["cur"][0].max()), *a["hist"][1:])
    kw = dict(motion=False, ids=False, clamp=True, clamp_gamma=gamma)
    out, length, _, _ = call_moments(hip.reproject_moments_host, a, shorten=True, shorten_rate=1.0, **kw)
    off = call_motion(hip.reproject_motion_host, a, **kw)
    R = call_moments(restate_moments, a, shorten=True, shorten_rate=1.0, **kw)
    n = 4.0
    assert (off[1] == 64).all() and (length >= n).all() and (length <= 1.01 * n).all()
    assert np.abs(length - R["length"]).max() <= 1e-5 * n and np.abs(out - R["out"]).max() <= 1e-5 * np.abs(R["out"]).max()
    # rate 0 shortens nothing: the clamp alone
    same_bits(call_moments(hip.reproject_moments_host, a, shorten=True, shorten_rate=0.0, **kw)[:2], off, "rate 0")


def test_a_lone_centre_and_a_bound_that_is_not_finite_shorten_nothing():
    a = mu_flat(seed=5)
    rgb, depth, ns = a["cur"]
    hrgb, hdepth, hlen = a["hist"]
    hrgb[...] = 40.0
    depth[9, 11] = hdepth[9, 11] = MISS      # a miss alone among hits: k == 1
    rgb[5, 5] = 3e38
    rgb[5, 6] = 3e38                         # their sum overflows: windows holding both have no finite mean
    kw = dict(motion=False, ids=False, clamp=True)
    out, length, _, _ = call_moments(hip.reproject_moments_host, a, shorten=True, shorten_rate=4.0, **kw)
    off = call_motion(hip.reproject_motion_host, a, motion=False, ids=False, clamp=False)
    spared = np.zeros(length.shape, bool)
    spared[9, 11] = True
    spared[4:7, 4:8] = True                  # (a window holding one of them has a finite mean and a deviation that overflows)
    same_bits((out[spared], length[spared]), (off[0][spared], off[1][spared]), "not clamped, not shortened")
    assert (length[spared] == 64).all() and (length[~spared] < 10).all() and np.isfinite(out).all()


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------

def test_refused_calls():
    a = moments_inputs(seed=9)
    rgb, depth, ns = a["cur"]
    hrgb, hdepth, hlen = a["hist"]
    hmom = a["hist_moments"]
    out, out_len = np.zeros((H, W, 3), np.float32), np.zeros((H, W), np.float32)
    om, ov = np.zeros((H, W, 2), np.float32), np.zeros((H, W), np.float32)
    table = np.zeros(3 * H * W // 16 + 16, hip.NODE_MOTION_DTYPE)
    table[:3] = a["motion"]
    c0, c1 = (np.array(c, dtype=hip.CAMERA_DTYPE).reshape(1) for c in (a["c0"], a["c1"]))
    P = hip.ReprojectMomentsParams
    good = dict(prev=c0.ctypes.data, cur=c1.ctypes.data, x0=0, y0=0, w=W, h=H, rgb=rgb.ctypes.data, depth=depth.ctypes.data, ns=ns.ctypes.data,
                ids=a["ids"].ctypes.data, hrgb=hrgb.ctypes.data, hdepth=hdepth.ctypes.data, hlen=hlen.ctypes.data, hids=a["hist_ids"].ctypes.data,
                hmom=hmom.ctypes.data, motion=table.ctypes.data, count=3, params=P.of(motion=True, clamp=True, moments=True, shorten=True),
                out=out.ctypes.data, out_len=out_len.ctypes.data, om=om.ctypes.data, ov=ov.ctypes.data)

    def rc(**change):
        g = dict(good, **change)
        r = hip.lib().qa_test_reproject_moments_host(*(C.byref(v) if isinstance(v, P) else v for v in g.values()))
        assert r == 0 or hip.lib().qa_last_error()
        return r

    assert rc() == 0 and rc(hmom=None) == 0
    # everything the old calls refuse
    for key in ("prev", "cur", "rgb", "depth", "ns", "hrgb", "hdepth", "hlen", "params", "out", "out_len"):
        assert rc(**{key: None}) == QA_EINVAL, key
    for change in (dict(w=0), dict(h=0), dict(w=-3), dict(x0=-1), dict(y0=-1), dict(x0=1 << 24), dict(w=1 << 16, h=1 << 16)):
        assert rc(**change) == QA_EINVAL, change
    for bad in (dict(depth_tolerance=-0.1), dict(depth_tolerance=float("nan")), dict(max_history=0.0), dict(max_history=float("inf"))):
        assert rc(params=P.of(**bad)) == QA_EINVAL, bad
    plain = P.default()
    assert rc(params=plain, ids=None) == QA_EINVAL and rc(params=plain, hids=None) == QA_EINVAL and rc(params=plain, ids=None, hids=None) == 0
    for change in (dict(out=good["hrgb"]), dict(out_len=good["hlen"]), dict(out_len=good["depth"]), dict(out=good["rgb"] + 12), dict(out_len=good["out"])):
        assert rc(**change) == QA_EINVAL, change
    for change in (dict(motion=None), dict(count=0), dict(ids=None, hids=None)):
        assert rc(params=P.of(motion=True), **change) == QA_EINVAL, change
    for bad in (dict(clamp_radius=0), dict(clamp_radius=4), dict(clamp_gamma=-0.5), dict(clamp_gamma=float("nan"))):
        assert rc(params=P.of(clamp=True, **bad)) == QA_EINVAL, bad
    assert rc(params=P.of(clamp=True), out=good["rgb"]) == QA_EINVAL and rc(params=P.of(moments=True), out=good["rgb"]) == 0
    assert rc(out=good["motion"]) == QA_EINVAL
    # unknown flag bits
    for flags in (16, 0x80000000, 31):
        p = P.default()
        p.flags = flags
        assert rc(params=p) == QA_EINVAL, flags
    # SHORTEN: only with CLAMP; a finite rate >= 0; without the flag the rate is not read
    assert rc(params=P.of(shorten=True)) == QA_EINVAL and rc(params=P.of(shorten=True, moments=True)) == QA_EINVAL
    for bad in (-0.5, float("nan"), float("inf")):
        assert rc(params=P.of(clamp=True, shorten=True, shorten_rate=bad)) == QA_EINVAL, bad
        assert rc(params=P.of(clamp=True, shorten_rate=bad)) == 0, bad
    assert rc(params=P.of(clamp=True, shorten=True, shorten_rate=0.0)) == 0
    # MOMENTS: both output planes, not the history's plane, nothing overlapping them, a finite min_frames >= 1
    only = P.of(moments=True)
    assert rc(params=only, om=None) == QA_EINVAL and rc(params=only, ov=None) == QA_EINVAL and rc(params=plain, om=None, ov=None) == 0
    assert rc(params=only, om=good["hmom"]) == QA_EINVAL and rc(params=only, ov=good["hmom"]) == QA_EINVAL
    for change in (dict(om=good["hrgb"]), dict(ov=good["hlen"]), dict(om=good["rgb"]), dict(ov=good["depth"]), dict(om=good["out"]), dict(ov=good["out_len"]),
                   dict(ov=good["om"] + 8), dict(om=good["om"] + 4), dict(out=good["hmom"]), dict(out_len=good["hmom"])):
        assert rc(params=only, **change) == QA_EINVAL, change
    assert rc(om=good["motion"]) == QA_EINVAL and rc(params=P.of(moments=True, clamp=True), om=good["motion"]) == 0
    for bad in (0.5, 0.0, -1.0, float("nan"), float("inf")):
        assert rc(params=P.of(moments=True, min_frames=bad)) == QA_EINVAL, bad
        assert rc(params=P.of(min_frames=bad)) == 0, bad
    assert rc(params=P.of(moments=True, min_frames=1.0)) == 0
    with pytest.raises(hip.HipError) as e:
        hip.reproject_moments_host(a["cur"], a["hist"], a["c0"], a["c1"], shorten=True)
    assert e.value.code == QA_EINVAL and "CLAMP" in str(e.value)
