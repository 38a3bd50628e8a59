"""Temporal reprojection on the CPU (qa_test_reproject_host: qaray_amd/csrc/hip/qa_reproject_dev.h built for the host) against a
float64 numpy restatement of the header's specification and against the analytic scene itself (tests/reproject_util.py): where the
history lands, what a disocclusion leaves, the properties that are exact, the inputs that must not make a NaN, the calls that are
refused.  No GPU: tests/test_gpu_reproject.py pins the kernel to this build bit for bit."""
import ctypes as C

import numpy as np
import pytest

import reproject_util as ru
from qaray_amd import hip
from reproject_util import BOUND, H, MISS, W, bits, call, frames, inputs, restate

QA_EINVAL = -1
UNDECIDED_CAP = 0.02


def host(a, ids=True, **kw):
    """hip.reproject_host on a dict of inputs(); the inputs are never written."""
    before = [np.array(x, copy=True) for x in (*a["cur"], *a["hist"], a["ids"], a["hist_ids"])]
    out, length = call(hip.reproject_host, a, ids, **kw)
    for x, y in zip(before, (*a["cur"], *a["hist"], a["ids"], a["hist_ids"])):
        assert np.array_equal(bits(x), bits(y))
    return out, length


def deviation(out, ref, mask):
    """The largest |out - ref| over the masked pixels as a fraction of the largest |ref| there."""
    if not mask.any():
        return 0.0
    return float(np.abs(out[mask] - ref[mask]).max() / max(np.abs(ref[mask]).max(), 1e-30))


@pytest.mark.parametrize("ids", (True, False))
def test_host_equals_the_restatement_on_decided_pixels(ids):
    a = inputs(seed=1)
    out, length = host(a, ids)
    R = call(restate, a, ids)
    assert R["undecided"].mean() <= UNDECIDED_CAP
    assert R["has"].mean() > 0.8 and (~R["has"] & R["hit"]).sum() > 50    # both branches are there
    dec = ~R["undecided"] & ~R["void"]
    dev, dev_len = deviation(out, R["out"], dec), deviation(length, R["length"], dec)
    print(f"ids {ids}: out deviates by {dev:.3g} of the largest component, length by {dev_len:.3g}; undecided {R['undecided'].mean():.4f}")
    assert dev <= BOUND and dev_len <= BOUND
    # the pixels without history and the void ones are exact
    none = dec & ~R["has"]
    assert np.array_equal(bits(out[none]), bits(a["cur"][0][none])) and np.array_equal(length[none], a["cur"][2][none].astype(np.float32))
    void = R["void"]
    assert void.sum() == 4 and np.array_equal(bits(out[void]), bits(a["cur"][0][void])) and not length[void].any()


def history_colour(hist_rgb, ids=True, shift_u=0.0):
    """c_h of views 0 -> 1 for a history colour: from `out` with a zero current colour, ns = 1, history length 63 and max_history
    64 (out = c_h * 63 / 64) -> (host c_h, host has, restatement)."""
    f = frames()
    a = dict(c0=f["c0"], c1=f["c1"], cur=(np.zeros((H, W, 3), np.float32), f["depth1"], np.ones((H, W), np.uint32)),
             hist=(np.ascontiguousarray(hist_rgb, np.float32), f["depth0"], np.full((H, W), 63, np.float32)), origin=(0, 0), ids=f["ids1"], hist_ids=f["ids0"])
    out, length = call(hip.reproject_host, a, ids, max_history=64)
    R = call(restate, a, ids, max_history=64, shift_u=shift_u)
    return out.astype(np.float64) * (64.0 / 63.0), length > 1.5, R


def test_history_lands_on_the_surface_point_it_was_rendered_at():
    f = frames()
    truth = ru.truth_colour(f["points1"])
    ch, has, R = history_colour(ru.truth_colour(f["points0"]))
    hit = f["depth1"] != MISS
    got = np.median(np.abs(ch - truth).max(-1)[has & hit])
    ref = np.median(np.abs(R["c_h"] - truth).max(-1)[R["has"] & hit])
    shifted = history_colour(ru.truth_colour(f["points0"]), shift_u=0.5)[2]
    off = np.median(np.abs(shifted["c_h"] - truth).max(-1)[shifted["has"] & hit])
    print(f"median |c_h - f(P)|: host {got:.3g}, restatement {ref:.3g}, restatement half a pixel off {off:.3g}")
    assert (has & hit).sum() > 2000
    assert got <= 4 * ref          # (bilinear interpolation of f over a slanted surface: 8.3e-5 in the restatement)
    assert off >= 10 * 4 * ref     # half a pixel off would be seen


def test_history_of_pixel_coordinates_returns_the_projection():
    px, py = np.meshgrid(np.arange(W), np.arange(H))
    ch, has, R = history_colour(np.stack([px / 64.0, py / 64.0, 0.0 * px], axis=-1))
    full = R["has"] & (R["taps"] == 4) & ~R["undecided"]
    assert full.sum() >= 0.6 * R["has"].sum()
    want = np.stack([R["u"], R["v"]], axis=-1)
    assert np.abs(ch[..., :2] * 64 - want)[full].max() <= BOUND * max(W, H)   # item 1's fraction of the largest component (66 / 64), in pixels


def test_disocclusions_lose_their_history():
    f = frames()
    zero_colour = np.zeros((H, W, 3))
    _, has, R = history_colour(zero_colour + 0.5)
    hit = f["depth1"] != MISS
    # (a) exact: pixels whose four taps all carry another id.  (Taps by the restatement's u, v, away from the integers.)
    fx, fy = R["ul"] - np.floor(R["ul"]), R["vl"] - np.floor(R["vl"])
    inner = hit & (R["ul"] >= 0) & (R["ul"] < W - 1) & (R["vl"] >= 0) & (R["vl"] < H - 1) & (fx > 0.01) & (fx < 0.99) & (fy > 0.01) & (fy < 0.99)
    i0, j0 = np.floor(np.where(inner, R["ul"], 0)).astype(int), np.floor(np.where(inner, R["vl"], 0)).astype(int)
    other = inner.copy()
    on_sphere = inner.copy()
    for dj in (0, 1):
        for di in (0, 1):
            tap = f["ids0"][j0 + dj, i0 + di]
            other &= (tap != f["ids1"]).any(-1)
            on_sphere &= tap[..., 0] == 2
    assert other.sum() >= 20 and not has[other].any()
    # (b), (c): against the analytic visibility of the pixel's point from C0
    visible = ru.visible_from(f["points1"], f["c0"])
    hidden = hit & ~visible
    print(f"hidden from C0: {hidden.sum()}, of which keep a history: {(hidden & has).sum()}")
    assert hidden.sum() >= 50 and (hidden & has).sum() <= 0.10 * hidden.sum()
    inside = hit & visible & (R["u"] >= 1) & (R["u"] <= W - 2) & (R["v"] >= 1) & (R["v"] <= H - 2)
    print(f"visible from C0 and inside: {inside.sum()}, of which lack a history: {(inside & ~has).sum()}")
    assert inside.sum() >= 2000 and (inside & ~has).sum() <= 0.02 * inside.sum()
    # (d) without ids the depth test alone rejects the sphere for a floor pixel behind it
    _, has_noids, _ = history_colour(zero_colour + 0.5, ids=False)
    floor_behind, wall_behind = on_sphere & (f["ids1"][..., 0] == 0), on_sphere & (f["ids1"][..., 0] == 1)
    print(f"all four taps on the sphere: {floor_behind.sum()} floor pixels, {wall_behind.sum()} wall pixels")
    assert floor_behind.sum() >= 3 and not has_noids[floor_behind].any() and not has_noids[wall_behind].any()
    # and a history plane of another id everywhere leaves every pixel as it came
    a = inputs(seed=3)
    a["hist_ids"][...] = 99
    out, length = host(a)
    assert np.array_equal(bits(out), bits(a["cur"][0]))


def test_still_camera_is_exact():
    a = inputs(seed=4, still=True)
    rgb, depth, ns = a["cur"]
    hrgb, hdepth, hlen = a["hist"]
    out, length = host(a, max_history=8)
    R = call(restate, a, max_history=8)
    assert not R["undecided"].any()
    c, ch = rgb, hrgb
    n = ns.astype(np.float32)
    L = np.minimum(hlen, np.float32(8))
    with np.errstate(all="ignore"):
        want = ch + (c - ch) * (n / (L + n))[..., None]
    assert want.dtype == np.float32
    has = R["has"]
    assert has.sum() == W * H - 4 - 2    # everything but the void pixels and the two without history
    assert np.array_equal(bits(out[has]), bits(want[has])) and np.array_equal(bits(length[has]), bits((L + n)[has]))
    assert np.array_equal(bits(out[~has]), bits(rgb[~has]))
    assert np.array_equal(length[~has], np.where(R["void"], 0, n)[~has])
    # a history that equals the colour comes back as the colour's bits, zero signs included
    b = inputs(seed=5, still=True)
    b["cur"][0][3, 3] = (-0.0, 0.0, 1.0)
    b["hist"] = (b["cur"][0].copy(), b["hist"][1], b["hist"][2])
    out, _ = host(b)
    assert np.array_equal(bits(out), bits(b["cur"][0]))


def test_pushes_without_motion_give_the_running_mean_and_the_length_saturates():
    f = frames()
    r = np.random.default_rng(6)
    acc, length = np.zeros((H, W, 3), np.float32), np.zeros((H, W), np.float32)
    ns = np.full((H, W), 4, np.uint32)
    shown = []
    for k in range(8):
        frame = r.random((H, W, 3), dtype=np.float32)
        shown.append(frame.astype(np.float64))
        acc, length = hip.reproject_host((frame, f["depth0"], ns), (acc, f["depth0"], length), f["c0"], f["c0"], ids=f["ids0"], hist_ids=f["ids0"])
        assert np.all(length == 4 * (k + 1))
        mean = np.mean(shown, axis=0)
        assert np.all(np.abs(acc - mean) <= 4 * np.spacing(mean.astype(np.float32)))
    for k in range(12):   # 32 + 4 * 12 > 64 + 4
        acc, length = hip.reproject_host((shown[0].astype(np.float32), f["depth0"], ns), (acc, f["depth0"], length), f["c0"], f["c0"])
    assert np.all(length == 64 + 4)
    out, length = hip.reproject_host((acc, f["depth0"], ns), (acc, f["depth0"], np.full((H, W), 1000, np.float32)), f["c0"], f["c1"], max_history=16)
    assert set(np.unique(length)) == {4.0, 20.0}
    # in place: the output over the current colour
    a = inputs(seed=8)
    want, _ = host(a)
    rgb = a["cur"][0]
    out, _ = hip.reproject_host(a["cur"], a["hist"], a["c0"], a["c1"], ids=a["ids"], hist_ids=a["hist_ids"], out=rgb)
    assert out is rgb and np.array_equal(bits(rgb), bits(want))


@pytest.mark.parametrize("name,a", ru.edge_cases(), ids=[n for n, _ in ru.edge_cases()])
def test_edges_make_no_nan_and_follow_the_restatement(name, a):
    for ids in (True, False):
        out, length = host(a, ids)
        R = call(restate, a, ids)
        assert np.isfinite(length).all() and np.isfinite(out[~R["void"]]).all()
        assert np.array_equal(bits(out[R["void"]]), bits(a["cur"][0][R["void"]]))
        if name.startswith("dof"):
            continue   # (the lens is not modelled: only finiteness, and device == host in tests/test_gpu_reproject.py)
        assert R["undecided"].mean() <= UNDECIDED_CAP or R["undecided"].size < 50
        dec = ~R["undecided"] & ~R["void"]
        assert np.array_equal((length > a["cur"][2])[dec], R["has"][dec])
        assert deviation(out, R["out"], dec) <= BOUND
        if name in ("c0 looks away", "pos0 on a hit point"):
            assert not R["has"].any()
        if name == "hit depth 1e29":
            far = a["cur"][1] == np.float32(1e29)
            assert far.sum() == 100 and not (length > 4)[far & ~R["void"]].any()


def test_refused_calls():
    a = inputs(seed=9)
    rgb, depth, ns = a["cur"]
    hrgb, hdepth, hlen = a["hist"]
    out, out_len = np.zeros((H, W, 3), np.float32), np.zeros((H, W), np.float32)
    c0, c1 = (np.array(c, dtype=hip.CAMERA_DTYPE).reshape(1) for c in (a["c0"], a["c1"]))
    good = dict(prev=c0.ctypes.data, cur=c1.ctypes.data, x0=0, y0=0, w=W, h=H, rgb=rgb.ctypes.data, depth=depth.ctypes.data, ns=ns.ctypes.data,
                ids=a["ids"].ctypes.data, hrgb=hrgb.ctypes.data, hdepth=hdepth.ctypes.data, hlen=hlen.ctypes.data, hids=a["hist_ids"].ctypes.data,
                params=hip.ReprojectParams.default(), out=out.ctypes.data, out_len=out_len.ctypes.data)

    def rc(**change):
        g = dict(good, **change)
        return hip.lib().qa_test_reproject_host(*(C.byref(v) if isinstance(v, hip.ReprojectParams) else v for v in g.values()))

    assert rc() == 0
    for key in ("prev", "cur", "rgb", "depth", "ns", "hrgb", "hdepth", "hlen", "params", "out", "out_len"):
        assert rc(**{key: None}) == QA_EINVAL, key
        assert hip.lib().qa_last_error()
    assert rc(ids=None) == QA_EINVAL and rc(hids=None) == QA_EINVAL and rc(ids=None, hids=None) == 0
    for change in (dict(w=0), dict(h=0), dict(w=-3), dict(x0=-1), dict(y0=-1), dict(x0=1 << 24), dict(w=1 << 16, h=1 << 16)):
        assert rc(**change) == QA_EINVAL, change
    for bad in (dict(depth_tolerance=-0.1), dict(depth_tolerance=float("nan")), dict(depth_tolerance=float("inf")), dict(max_history=0.0),
                dict(max_history=-1.0), dict(max_history=float("nan")), dict(max_history=float("inf"))):
        assert rc(params=hip.ReprojectParams.of(**bad)) == QA_EINVAL, bad
    p = hip.ReprojectParams.default()
    p.flags = 1
    assert rc(params=p) == QA_EINVAL
    assert (p.depth_tolerance, p.max_history) == (np.float32(0.05), 64.0)
    # aliasing: the colour may be written in place, nothing else may overlap, and never a history plane
    assert rc(out=good["rgb"]) == 0
    for change in (dict(out=good["hrgb"]), dict(out_len=good["hlen"]), dict(out_len=good["hdepth"]), dict(out=good["hrgb"] + 12), dict(out_len=good["hids"]),
                   dict(out_len=good["depth"]), dict(out_len=good["ns"]), dict(out=good["rgb"] + 12), dict(out_len=good["out"]), dict(out=good["ids"])):
        assert rc(**change) == QA_EINVAL, change
    with pytest.raises(hip.HipError) as e:
        hip.reproject_host(a["cur"], a["hist"], a["c0"], a["c1"], ids=a["ids"])
    assert e.value.code == QA_EINVAL and "ids" in str(e.value)
