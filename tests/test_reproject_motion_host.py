"""Reprojection with node motion and colour clamp on the CPU (qa_test_reproject_motion_host and qa_reproject_node_motion:
qaray_amd/csrc/hip/qa_reproject_motion_dev.h built for the host) against the form it extends, against a float64 numpy restatement
of the header's specification and against the analytic scene with a sphere that moves (tests/reproject_motion_util.py).  No GPU:
tests/test_gpu_reproject_motion.py pins the kernel to this build bit for bit."""
import ctypes as C

import numpy as np
import pytest

import reproject_motion_util as mu
import reproject_util as ru
from qaray_amd import hip
from reproject_motion_util import call_motion, motion_inputs, moved_frames, restate_motion
from reproject_util import H, MISS, W, bits, call, inputs

QA_EINVAL = -1
UNDECIDED_CAP = 0.02


def same_bits(got, want, what):
    for g, w, name in zip(got, want, ("out", "length")):
        bad = np.argwhere(bits(g) != bits(w))
        assert bad.size == 0, (what, name, len(bad), bad[:5])


def deviation(out, ref, mask):
    return float(np.abs(out[mask] - ref[mask]).max() / max(np.abs(ref[mask]).max(), 1e-30)) if mask.any() else 0.0


# ---- 1. flags 0: the old form's bits ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("still", (False, True))
@pytest.mark.parametrize("size,origin", (((W, H), (0, 0)), ((62, 42), (5, 3))))
def test_flags_0_give_the_old_forms_bits(size, origin, still):
    a = inputs(size[0], size[1], origin, seed=2, still=still)
    for ids in (True, False):
        want = call(hip.reproject_host, a, ids)
        same_bits(call(hip.reproject_motion_host, a, ids), want, (ids,))
        same_bits(call(hip.reproject_motion_host, a, ids, max_history=8, depth_tolerance=0.2), call(hip.reproject_host, a, ids, max_history=8, depth_tolerance=0.2),
                  (ids, "parameters"))


@pytest.mark.parametrize("name,a", ru.edge_cases(), ids=[n for n, _ in ru.edge_cases()])
def test_flags_0_give_the_old_forms_bits_on_the_edge_cases(name, a):
    for ids in (True, False):
        same_bits(call(hip.reproject_motion_host, a, ids), call(hip.reproject_host, a, ids), (name, ids))


def test_defaults():
    p = hip.ReprojectMotionParams.default()
    assert (p.depth_tolerance, p.max_history, p.flags) == (np.float32(0.05), 64.0, 0)
    assert (p.clamp_radius, p.clamp_gamma) == (1, 1.0)    # the table behind the two
    assert hip.NODE_MOTION_DTYPE.itemsize == 64 and (hip.QA_REPROJECT_MOTION, hip.QA_REPROJECT_CLAMP) == (1, 2)


# ---- 2. qa_reproject_node_motion -------------------------------------------------------------------------------------------------

CHAIN_PARENTS = [-1, 0, 1, 2, 0, 4]    # root; a chain of three below it; a sibling of the chain's first node and its child


def chain_tables(seed=0):
    r = np.random.default_rng(seed)

    def place():
        return mu.rotation(r.normal(size=3), r.uniform(-180, 180)) * r.uniform(0.5, 2.0), r.uniform(-3, 3, 3)

    prev = [mu.IDENTITY] + [place() for _ in range(5)]
    cur = list(prev)
    cur[1] = place()
    return mu.instance_table(prev, CHAIN_PARENTS), mu.instance_table(cur, CHAIN_PARENTS)


def test_node_motion_of_equal_tables_is_the_exact_identity():
    prev, _ = chain_tables()
    m = hip.node_motion(prev, prev.copy())
    assert m.dtype == hip.NODE_MOTION_DTYPE and len(m) == 6 and not m["moved"].any() and not m["pad"].any()
    assert np.array_equal(bits(m["m"]), bits(np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32), (6, 1))))


def test_a_moved_parent_marks_its_subtree_and_nothing_else():
    prev, cur = chain_tables()
    m = hip.node_motion(prev, cur)
    assert m["moved"].tolist() == [0, 1, 1, 1, 0, 0]
    ident = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32)
    assert all(np.array_equal(bits(m["m"][k]), bits(ident)) for k in (0, 4, 5))
    # a change of itm alone, of the last bit, marks the node too
    cur2 = prev.copy()
    cur2["itm"][5, 3] = np.nextafter(cur2["itm"][5, 3], np.float32(9))
    assert hip.node_motion(prev, cur2)["moved"].tolist() == [0, 0, 0, 0, 0, 1]


def test_node_motion_takes_current_points_to_where_they_were():
    prev, cur = chain_tables()
    m = hip.node_motion(prev, cur)
    p = np.random.default_rng(1).uniform(-3, 3, (500, 3))
    worst, ident = 0.0, 0.0
    for k in (1, 2, 3):
        now, before = mu.world(cur, k, p), mu.world(prev, k, p)
        M = np.asarray(m["m"][k], np.float64)
        got = now @ M[:9].reshape(3, 3).T + M[9:]
        worst = max(worst, float(np.abs(got - before).max() / np.abs(before).max()))
        ident = max(ident, float(np.abs(now - before).max() / np.abs(before).max()))
    print(f"|M_k Wcur(k)(p) - Wprev(k)(p)| / max|Wprev(k)(p)|: {worst:.3g} (with the identity in M's place: {ident:.3g})")
    assert worst <= mu.NODE_MOTION_BOUND and ident > 0.1


def test_node_motion_refuses_tables_of_different_graphs():
    prev, cur = chain_tables()
    for field, k, v in (("parent", 5, 0), ("subtree_end", 1, 3), ("depth", 2, 1)):
        bad = cur.copy()
        bad[field][k] = v
        with pytest.raises(hip.HipError) as e:
            hip.node_motion(prev, bad)
        assert e.value.code == QA_EINVAL, field
    both = prev.copy()
    both["parent"][2] = 3    # the same in both tables, but no pre-order
    with pytest.raises(hip.HipError):
        hip.node_motion(both, both.copy())
    L = hip.lib()
    out = np.zeros(6, hip.NODE_MOTION_DTYPE)
    for args in ((None, cur.ctypes.data, 6, out.ctypes.data), (prev.ctypes.data, None, 6, out.ctypes.data), (prev.ctypes.data, cur.ctypes.data, 6, None),
                 (prev.ctypes.data, cur.ctypes.data, 0, out.ctypes.data)):
        assert L.qa_reproject_node_motion(*args) == QA_EINVAL and L.qa_last_error()


# ---- 3. the moved sphere ---------------------------------------------------------------------------------------------------------

def moved_history_colour(still, identity_motion=False):
    """c_h of the scene before -> after the sphere's move, for a history colour that is a linear function of the object-local position
    on the sphere and of the world position elsewhere: from `out` with a zero current colour, ns = 1, history length 63
    (out = c_h * 63 / 64) -> (host c_h, host has, restatement, the colour every current pixel's point had)."""
    f = moved_frames(still)
    on0, on1 = f["ids0"][..., 0] == 2, f["ids1"][..., 0] == 2
    hist_rgb = np.where(on0[..., None], mu.local_colour(mu.sphere_local(f["points0"], mu.SPHERE_PREV)), ru.truth_colour(f["points0"]))
    truth = np.where(on1[..., None], mu.local_colour(mu.sphere_local(f["points1"], mu.SPHERE_CUR)), ru.truth_colour(f["points1"]))
    a = dict(c0=f["c0"], c1=f["c1"], cur=(np.zeros((H, W, 3), np.float32), f["depth1"], np.ones((H, W), np.uint32)),
             hist=(hist_rgb.astype(np.float32), f["depth0"], np.full((H, W), 63, np.float32)), origin=(0, 0), ids=f["ids1"], hist_ids=f["ids0"],
             motion=f["motion"])
    out, length = call_motion(hip.reproject_motion_host, a, max_history=64)
    R = call_motion(restate_motion, a, max_history=64, identity_motion=identity_motion)
    return out.astype(np.float64) * (64.0 / 63.0), length > 1.5, R, truth


@pytest.mark.parametrize("still", (True, False), ids=("still camera", "moving camera"))
def test_the_history_of_a_moved_node_is_fetched_from_where_it_was(still):
    """Measured: median |c_h - f| over the sphere's pixels with history 2.45e-3 (host and restatement alike; bilinear interpolation of
    a linear f over a curved surface) with a still camera and 2.89e-3 with a moving one; with the identity in M's place 0.424 / 0.421.
    Uncovered pixels that keep a history: 0 of 71 / 4 of 143; unmoved visible pixels inside that lack one: 0 of 2425 / 15 of 2318."""
    f = moved_frames(still)
    assert f["motion"]["moved"].tolist() == [0, 0, 1]
    ch, has, R, truth = moved_history_colour(still)
    sphere = f["ids1"][..., 0] == 2
    hit = f["depth1"] != MISS
    err = np.abs(ch - truth).max(-1)
    got = np.median(err[sphere & has])
    ref = np.median(np.abs(R["c_h"] - truth).max(-1)[sphere & R["has"]])
    Ri = moved_history_colour(still, identity_motion=True)[2]
    off = np.median(np.abs(Ri["c_h"] - truth).max(-1)[sphere & Ri["has"]])
    print(f"sphere pixels {sphere.sum()}, with history {(sphere & has).sum()} (restatement {(sphere & R['has']).sum()}); median |c_h - f|: host {got:.3g}, "
          f"restatement {ref:.3g}, restatement with the identity for M {off:.3g}")
    assert np.array_equal(R["moved"], sphere)
    assert (sphere & has).sum() >= 0.6 * sphere.sum() and (sphere & R["has"]).sum() >= 0.6 * sphere.sum()
    assert got <= 4 * ref
    assert off >= 10 * 4 * ref    # a history fetched from where the sphere now is would be seen
    # what the sphere uncovered: floor and wall points that the sphere, where it stood, hid from the old camera
    uncovered = hit & ~sphere & mu.hidden_by_sphere(f["points1"], f["c0"], mu.SPHERE_PREV[1])
    for name, keeps in (("host", has), ("restatement", R["has"])):
        print(f"uncovered by the sphere: {uncovered.sum()}, of which keep a history ({name}): {(uncovered & keeps).sum()}")
        assert uncovered.sum() >= 50 and (uncovered & keeps).sum() <= 0.10 * uncovered.sum()
    inside = hit & ~sphere & ~uncovered & (R["u"] >= 1) & (R["u"] <= W - 2) & (R["v"] >= 1) & (R["v"] <= H - 2)
    for name, keeps in (("host", has), ("restatement", R["has"])):
        print(f"unmoved, visible from the old camera and inside: {inside.sum()}, of which lack a history ({name}): {(inside & ~keeps).sum()}")
        assert inside.sum() >= 1500 and (inside & ~keeps).sum() <= 0.02 * inside.sum()
    # and the unmoved pixels land on their surface point as before
    rest = hit & ~sphere & has
    assert np.median(err[rest]) <= 4 * max(np.median(np.abs(R["c_h"] - truth).max(-1)[hit & ~sphere & R["has"]]), 1e-7)


def test_ids_outside_the_table_are_unmoved_nodes():
    a = motion_inputs(seed=3)
    a["ids"][0:20, :, 0] = np.array([-1, 3, 10, np.iinfo(np.int32).min], np.int32)[np.arange(W) % 4]
    a["hist_ids"][0:20] = a["ids"][0:20]
    short = dict(a, motion=a["motion"][:2])    # the sphere's record is beyond the table: nothing moves
    none_moved = a["motion"].copy()
    none_moved["moved"] = 0
    same_bits(call_motion(hip.reproject_motion_host, short), call_motion(hip.reproject_motion_host, dict(a, motion=none_moved)), "short table")
    same_bits(call_motion(hip.reproject_motion_host, short), call(hip.reproject_host, a), "no moved node: the old form")
    assert (bits(call_motion(hip.reproject_motion_host, a)[0]) != bits(call(hip.reproject_host, a)[0])).any()


# ---- 4. the clamp ----------------------------------------------------------------------------------------------------------------

K16 = dict(ns=4, length=60.0)    # out = c_h + (c - c_h) / 16, so c_h = (16 out - c) / 15


def flat_inputs(seed=0, w=23, h=19):
    """A still camera over a surface of constant depth: every pixel reprojects onto itself with one tap of weight 1, so c_h is the
    history pixel itself (and what the clamp made of it)."""
    r = np.random.default_rng(seed)
    c = ru.cam0()
    return dict(c0=c, c1=c, cur=(r.random((h, w, 3), dtype=np.float32) + np.float32(0.5), np.full((h, w), 5, np.float32), np.full((h, w), K16["ns"], np.uint32)),
                hist=(np.zeros((h, w, 3), np.float32), np.full((h, w), 5, np.float32), np.full((h, w), K16["length"], np.float32)), origin=(0, 0), ids=None,
                hist_ids=None, motion=None)


def clamped(a, **kw):
    """-> (host c_h recovered from out in float64, host out, host out with the clamp off, restatement)."""
    out, _ = call_motion(hip.reproject_motion_host, a, motion=False, ids=False, clamp=True, **kw)
    off, _ = call_motion(hip.reproject_motion_host, a, motion=False, ids=False, clamp=False)
    R = call_motion(restate_motion, a, motion=False, ids=False, clamp=True, **kw)
    with np.errstate(invalid="ignore"):   # (a void pixel's colour may be infinite)
        ch = (16.0 * out.astype(np.float64) - a["cur"][0].astype(np.float64)) / 15.0
    return ch, out, off, R


def tolerance(R):
    """Float32 against float64 in a bound of the box: sums of at most 49 terms, a division, a square root and a product - each term
    and step within 2^-24 of its value, so within 64 * 2^-24 = 3.8e-6 of the largest value in play; c_h is recovered from `out`
    through 16 out - c, which adds 17 * 2^-24 of it.  1e-5 of the largest |bound| covers both."""
    return 1e-5 * float(max(np.abs(R["lo"]).max(), np.abs(R["hi"]).max(), 1.0))


@pytest.mark.parametrize("r", (1, 2, 3))
def test_a_history_at_the_window_mean_is_not_touched(r):
    a = flat_inputs(seed=r)
    _, mean, _, _ = mu.window_stats(*a["cur"], r)
    a["hist"] = (mean.astype(np.float32), *a["hist"][1:])
    _, out, off, R = clamped(a, clamp_radius=r, clamp_gamma=1.0)
    assert R["box"].all() and np.array_equal(bits(out), bits(off))


@pytest.mark.parametrize("gamma", (0.0, 1.0, 2.5))
@pytest.mark.parametrize("r", (1, 2, 3))
def test_a_far_history_comes_back_on_the_box_and_windows_are_clipped_at_the_border(r, gamma):
    a = flat_inputs(seed=10 + r)
    a["hist"] = (np.full_like(a["cur"][0], 100 * a["cur"][0].max()), *a["hist"][1:])
    ch, out, off, R = clamped(a, clamp_radius=r, clamp_gamma=gamma)
    h, w = R["k"].shape
    assert R["k"][0, 0] == (r + 1) ** 2 and R["k"][h - 1, w // 2] == (r + 1) * (2 * r + 1) and R["k"][h // 2, w // 2] == (2 * r + 1) ** 2
    tol = tolerance(R)
    assert (ch >= R["lo"] - tol).all() and (ch <= R["hi"] + tol).all()
    assert np.abs(ch - R["hi"]).max() <= tol    # ... at the upper bound, corners and edges included
    assert np.abs(out - R["out"]).max() <= tol
    assert (off > 50).all()                    # the clamp-off call keeps the history as it is
    if gamma == 0.0:
        assert np.abs(ch - mu.window_stats(*a["cur"], r)[1]).max() <= tol
    low = dict(a, hist=(np.full_like(a["cur"][0], -100.0), *a["hist"][1:]))
    ch, _, _, R = clamped(low, clamp_radius=r, clamp_gamma=gamma)
    assert np.abs(ch - R["lo"]).max() <= tol


@pytest.mark.parametrize("r", (1, 3))
def test_a_constant_window_clamps_to_its_mean_exactly(r):
    a = flat_inputs()
    a["cur"][0][...] = np.float32(0.375)
    a["hist"][0][...] = 7.0
    _, out, off, R = clamped(a, clamp_radius=r, clamp_gamma=3.0)
    assert np.array_equal(bits(out), bits(a["cur"][0])) and (off > 6).all()    # c_h == m == c: the colour's own bits


def test_lone_centres_void_pixels_and_other_classes():
    a = flat_inputs(seed=5)
    rgb, depth, ns = a["cur"]
    hrgb, hdepth, hlen = a["hist"]
    hrgb[...] = 40.0
    # (a) a miss pixel alone among hits, its history a miss too: k == 1, not clamped
    depth[9, 11] = hdepth[9, 11] = MISS
    # (b) void neighbours and a block of misses with huge colours: they must not widen a hit pixel's box
    ns[3, 3] = 0
    rgb[3, 3] = 1e6
    rgb[4, 5, 1] = np.inf
    depth[12:15, 2:5] = hdepth[12:15, 2:5] = MISS
    rgb[12:15, 2:5] = 5e5
    ch, out, off, R = clamped(a, clamp_radius=2, clamp_gamma=1.0)
    assert R["k"][9, 11] == 1 and not R["box"][9, 11] and np.array_equal(bits(out[9, 11]), bits(off[9, 11])) and off[9, 11, 0] > 30
    hit = R["hit"]
    assert R["hi"][hit].max() < 2.0    # (colours of 0.5 .. 1.5: no huge neighbour entered a hit pixel's window)
    tol = tolerance(dict(lo=R["lo"][hit], hi=R["hi"][hit]))
    assert np.abs(ch - R["hi"])[hit].max() <= tol
    block = np.zeros_like(hit)
    block[12:15, 2:5] = True
    assert (R["k"][block] == 9).all() and np.abs(ch[block] - 5e5).max() <= 5.0    # the misses' own box, 5e5 +- 0: no hit pixel of about 1 in it
    void = R["void"]
    assert void.sum() == 2 and np.array_equal(bits(out[void]), bits(rgb[void]))


def test_a_bound_that_is_not_finite_clamps_nothing():
    a = flat_inputs(seed=6)
    a["cur"][0][5, 5] = 3e38
    a["cur"][0][5, 6] = 3e38     # the sum of the two overflows: windows holding both have no finite mean
    a["hist"][0][...] = 40.0
    ch, out, off, R = clamped(a, clamp_radius=1, clamp_gamma=1.0)
    both = np.zeros(R["k"].shape, bool)
    both[4:7, 5:7] = True
    assert np.array_equal(bits(out[both]), bits(off[both]))
    assert np.isfinite(out).all()


# ---- 5. both flags against the restatement -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("still", (False, True))
def test_host_equals_the_restatement_with_both_flags(still):
    """The clamp's own comparisons (c_h against lo and hi) are no decisions in the sense of `undecided`: the clamped value is a
    continuous function of c_h and the bounds, so taking one the other way moves the result by the rounding error alone."""
    a = motion_inputs(seed=1, still=still)
    kw = dict(clamp=True, clamp_radius=2, clamp_gamma=1.0)
    before = [np.array(x, copy=True) for x in (*a["cur"], *a["hist"], a["ids"], a["hist_ids"])]
    out, length = call_motion(hip.reproject_motion_host, a, **kw)
    for x, y in zip(before, (*a["cur"], *a["hist"], a["ids"], a["hist_ids"])):
        assert np.array_equal(bits(x), bits(y))
    R = call_motion(restate_motion, a, **kw)
    assert R["undecided"].mean() <= UNDECIDED_CAP
    assert R["moved"].sum() > 200 and (R["moved"] & R["has"]).sum() > 100 and (R["box"] & (R["c_h"] != R["unclamped"]).any(-1)).sum() > 1000
    dec = ~R["undecided"] & ~R["void"]
    dev, dev_len = deviation(out, R["out"], dec), deviation(length, R["length"], dec)
    print(f"still {still}: out deviates by {dev:.3g} of the largest component, length by {dev_len:.3g}; undecided {R['undecided'].mean():.4f}")
    assert dev <= mu.BOTH_BOUND and dev_len <= mu.BOTH_BOUND
    assert np.array_equal((length > a["cur"][2])[dec], R["has"][dec])
    none = dec & ~R["has"]
    assert np.array_equal(bits(out[none]), bits(a["cur"][0][none]))
    # the length is the clamp-off call's
    assert np.array_equal(bits(length), bits(call_motion(hip.reproject_motion_host, a)[1]))


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------

def test_refused_calls():
    a = motion_inputs(seed=9)
    rgb, depth, ns = a["cur"]
    hrgb, hdepth, hlen = a["hist"]
    out, out_len = np.zeros((H, W, 3), np.float32), np.zeros((H, W), np.float32)
    table = np.zeros(3 * H * W // 16 + 16, hip.NODE_MOTION_DTYPE)    # (large enough to stand in for an output plane)
    table[:3] = a["motion"]
    c0, c1 = (np.array(c, dtype=hip.CAMERA_DTYPE).reshape(1) for c in (a["c0"], a["c1"]))
    P = hip.ReprojectMotionParams
    good = dict(prev=c0.ctypes.data, cur=c1.ctypes.data, x0=0, y0=0, w=W, h=H, rgb=rgb.ctypes.data, depth=depth.ctypes.data, ns=ns.ctypes.data,
                ids=a["ids"].ctypes.data, hrgb=hrgb.ctypes.data, hdepth=hdepth.ctypes.data, hlen=hlen.ctypes.data, hids=a["hist_ids"].ctypes.data,
                motion=table.ctypes.data, count=3, params=P.of(motion=True, clamp=True), out=out.ctypes.data, out_len=out_len.ctypes.data)

    def rc(**change):
        g = dict(good, **change)
        r = hip.lib().qa_test_reproject_motion_host(*(C.byref(v) if isinstance(v, P) else v for v in g.values()))
        assert r == 0 or hip.lib().qa_last_error()
        return r

    assert rc() == 0
    # everything the old call refuses
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
    # unknown flag bits
    for flags in (4, 8, 0x80000000, 7):
        p = P.default()
        p.flags = flags
        assert rc(params=p) == QA_EINVAL, flags
    # the motion flag: a null table, count < 1, not both ids planes; without the flag none of them matters
    only_motion = P.of(motion=True)
    for change in (dict(motion=None), dict(count=0), dict(count=-2), dict(ids=None, hids=None), dict(ids=None), dict(hids=None)):
        assert rc(params=only_motion, **change) == QA_EINVAL, change
    assert rc(params=plain, motion=None, count=0) == 0 and rc(params=P.of(clamp=True), motion=None, count=0, ids=None, hids=None) == 0
    # the clamp flag: radius 1 .. 3, a finite gamma >= 0, not in place; without the flag none of them matters
    for bad in (dict(clamp_radius=0), dict(clamp_radius=4), dict(clamp_radius=-1), dict(clamp_gamma=-0.5), dict(clamp_gamma=float("nan")),
                dict(clamp_gamma=float("inf"))):
        assert rc(params=P.of(clamp=True, **bad)) == QA_EINVAL, bad
        assert rc(params=P.of(motion=True, **bad)) == 0, bad
    assert rc(params=P.of(clamp=True, clamp_gamma=0.0, clamp_radius=3)) == 0
    assert rc(params=P.of(clamp=True), out=good["rgb"]) == QA_EINVAL and rc(params=only_motion, out=good["rgb"]) == 0
    # an output over the motion table
    assert rc(out=good["motion"]) == QA_EINVAL and rc(out_len=good["motion"] + 64) == QA_EINVAL
    with pytest.raises(hip.HipError) as e:
        hip.reproject_motion_host(a["cur"], a["hist"], a["c0"], a["c1"], motion=a["motion"])
    assert e.value.code == QA_EINVAL and "ids" in str(e.value)
