"""Ambient occlusion (qa_ao_region*, qa_progressive_ao_device, qa_ao_points*: qa_ao.hip; the opening comment of qa_ao_dev.h is the
specification) against the composition of the public queries it fuses: the camera rays of every sample handed out
(camera_sample_rays_device), cast as rays of the caller's (cast_rays_device), the facing normals and the directions made on the host
from the source the kernels are compiled from (held to a numpy restatement by tests/test_ao_host.py), and every shadow ray tested by
occluded_device - all of them pinned to the CPU oracle by their own tests.  The planes are integers: every comparison is exact, on
every pixel.

Frames of 64x48 (gbuffer_util): the Cornell box (the LDS-resident kernel), the probe camera box_edge (misses and hits in one tile),
sphere_inside (every hit on a back face), the teapot (a mesh in global memory) and texedge_big.xml (textured, global memory)."""
import functools
import os

import numpy as np
import pytest

from conftest import GOLDEN
from ao_util import F32, ao_ref, bits, differing, extent_of, first_hits, planes_numpy, route, samples_ref, stream_ids
from gbuffer_util import REGION, SEEDS, SIZE, scene_blob
from ray_query_util import BOX, QA_BIAS, TEAPOT, dof_blob, fresh, probe_blob

pytestmark = pytest.mark.gpu
QA_EINVAL, QA_ENOSCENE, QA_EUNSUPPORTED = -1, -5, -6
TEXTURED_GLOBAL = os.path.join(GOLDEN, "texedge", "texedge_big.xml")
FRAMES = ("box", "box_edge", "sphere_inside", "teapot", "textured_global")
SPP, K = 3, 4
FIRSTS = (0, 2)
RAGGED = (7, 5, 26, 18)     # 19 x 13 at an odd origin
ONE = (31, 22, 32, 23)
REGIONS = {"region": REGION, "ragged": RAGGED, "one": ONE}
W = SIZE[0]
INF = float("inf")
EDGE_RADIUS = 10.0   # box_edge: at a tenth of the extent every ray of that frame is open; at this radius some are and some are not (asserted)


@functools.lru_cache(maxsize=None)
def blob_of(frame):
    if frame in ("box_edge", "sphere_inside"):
        return probe_blob(frame)
    return scene_blob({"box": BOX, "teapot": TEAPOT, "textured_global": TEXTURED_GLOBAL}[frame])


def device_planes(c, *args, **kw):
    out = c.ao_device(*args, **kw)
    c.synchronize()
    return planes_numpy(out)


@pytest.fixture(scope="module")
def frames():
    """frame -> dict: "name" the kernel's; "radii" the three radii (unbounded, a tenth of the extent, twice the bias); ("hits", region,
    first) the first hits of the composition; ("want" / "got", region, first, radius index) the composition's and the fused call's planes"""
    out = {}
    for frame in FRAMES:
        c = fresh(blob_of(frame))
        try:
            d = {"name": c.kernel_name()}
            whole = first_hits(c, REGION, 0, SPP)
            d["radii"] = (INF, extent_of(whole) / 10.0, 2.0 * float(QA_BIAS))
            for rname, region in REGIONS.items():
                for first in FIRSTS:
                    hits = whole if (rname, first) == ("region", 0) else first_hits(c, region, first, SPP)
                    d["hits", rname, first] = hits
                    for i, radius in enumerate(d["radii"]):
                        d["want", rname, first, i] = route(c, region, W, first, SPP, K, radius, SEEDS[0], hits=hits)
                        d["got", rname, first, i] = device_planes(c, region, SPP, K, radius, first=first, seed=SEEDS[0])
            out[frame] = d
        finally:
            c.close()
    return out


def test_the_frames_show_what_they_are_chosen_for(frames):
    assert "RES=1" in frames["box"]["name"] and "RES=0" in frames["teapot"]["name"]
    assert "RES=0" in frames["textured_global"]["name"] and "TEX=1" in frames["textured_global"]["name"]
    edge = frames["box_edge"]["hits", "region", 0]["hit"]
    tiles = [edge[y:y + 8, x:x + 8] for y in range(0, 40, 8) for x in range(0, 40, 8)]
    assert any(t.any() and not t.all() for t in tiles), "box_edge: no tile with hits and misses"
    inside = frames["sphere_inside"]["hits", "region", 0]
    along = (inside["N"].astype(np.float64) * inside["dirs"]).sum(axis=-1)[inside["hit"]]
    assert inside["hit"].all() and (along > 0).all(), "sphere_inside: a hit on a front face"
    assert np.array_equal(inside["normal"], -inside["N"])
    for frame in FRAMES:
        r = frames[frame]["radii"]
        print(frame, frames[frame]["name"], "radii", r)
        assert r[0] > r[1] > r[2] > float(QA_BIAS)


@pytest.mark.parametrize("frame", FRAMES)
def test_the_fused_call_is_the_composition_on_every_pixel(frames, frame):
    d = frames[frame]
    seen_open = seen_closed = False
    for rname, region in REGIONS.items():
        h, w = region[3] - region[1], region[2] - region[0]
        for first in FIRSTS:
            for i in range(3):
                got, want = d["got", rname, first, i], d["want", rname, first, i]
                assert got["open"].shape == (h, w) and got["open"].dtype == np.uint32 and got["ao"].dtype == F32
                assert not differing(got, want), (frame, rname, first, i, differing(got, want), int((got["open"] != want["open"]).sum()))
                assert np.array_equal(bits(got["ao"]), bits(ao_ref(got["open"], got["rays"])))
                assert np.array_equal(got["rays"], d["hits", rname, first]["hit"].sum(axis=2) * K)
                seen_open |= bool((got["open"] > 0).any())
                seen_closed |= bool((got["open"] < got["rays"]).any())
    assert seen_open and seen_closed, "the frame shows no open ray, or no occluded one: the comparison would pass on a constant"
    # twice the bias: a ray that short meets nothing but a surface it starts on
    short = d["got", "region", 0, 2]
    print(frame, "open / rays: unbounded", d["got", "region", 0, 0]["open"].sum(), "a tenth", d["got", "region", 0, 1]["open"].sum(), "twice the bias",
          short["open"].sum(), "of", short["rays"].sum())


@pytest.mark.parametrize("frame", FRAMES)
def test_open_falls_as_the_radius_grows(frames, frame):
    """Exact, from the definition of shadow: what a ray meets before r1 it meets before r2 > r1"""
    for first in FIRSTS:
        unbounded, tenth, short = (frames[frame]["got", "region", first, i] for i in range(3))
        assert (short["open"] >= tenth["open"]).all() and (tenth["open"] >= unbounded["open"]).all()
        assert np.array_equal(short["rays"], tenth["rays"]) and np.array_equal(tenth["rays"], unbounded["rays"])


@pytest.mark.parametrize("frame", ("box_edge", "teapot"))
def test_sample_ranges_add_up(frames, frame):
    import torch
    c = fresh(blob_of(frame))
    try:
        radius = frames[frame]["radii"][1]
        whole = device_planes(c, REGION, 4, K, radius, first=0)
        a, b = device_planes(c, REGION, 2, K, radius, first=0), device_planes(c, REGION, 2, K, radius, first=2)
        assert np.array_equal(whole["open"], a["open"] + b["open"]) and np.array_equal(whole["rays"], a["rays"] + b["rays"])
        assert whole["rays"].max() == 4 * K and (whole["open"] > 0).any()
        # the host form and a single plane are the device form's
        host = c.ao(REGION, 4, K, radius)
        assert not differing(host, whole)
        one = device_planes(c, REGION, 4, K, radius, ao=torch.empty((40, 47), dtype=torch.float32, device="cuda:0"))
        assert list(one) == ["ao"] and np.array_equal(bits(one["ao"]), bits(whole["ao"]))
    finally:
        c.close()


@pytest.mark.parametrize("first", FIRSTS)
def test_an_ns_plane_gives_each_pixel_its_own_count(frames, first):
    import torch
    h, w = REGION[3] - REGION[1], REGION[2] - REGION[0]
    values = np.array([0, 1, SPP, SPP + 5], np.uint32)
    ns = values[(np.arange(h)[:, None] * 3 + np.arange(w)[None, :]) % 4]
    assert all(set(ns[y:y + 8, x:x + 8].ravel().tolist()) == set(values.tolist()) for y in range(0, h - 7, 8) for x in range(0, w - 7, 8))
    n = samples_ref(ns, first, SPP)
    radius = EDGE_RADIUS
    c = fresh(blob_of("box_edge"))
    try:
        got = device_planes(c, REGION, SPP, K, radius, first=first, ns=torch.from_numpy(ns.view(np.int32)).cuda())
        assert (got["open"] > 0).any() and (got["open"] < got["rays"]).any()
        seen = set()
        for count in np.unique(n).tolist():
            at = n == count
            seen.add(count)
            if count == 0:
                assert not got["open"][at].any() and not got["rays"][at].any() and (got["ao"][at] == 1).all()
                continue
            own = device_planes(c, REGION, count, K, radius, first=first)
            for k in ("open", "rays", "ao"):
                assert np.array_equal(bits(got[k])[at], bits(own[k])[at]), (count, k)
        assert seen == {0, 1, SPP}, seen
        # and the composition agrees
        want = route(c, REGION, W, first, SPP, K, radius, SEEDS[0], n=n, hits=frames["box_edge"]["hits", "region", first])
        assert not differing(got, want)
        assert not differing(c.ao(REGION, SPP, K, radius, first=first, ns=ns), got)
    finally:
        c.close()


def test_the_progressive_form_follows_the_frames_own_counts_and_seed():
    import torch
    region, spp, spp_max, seed = (8, 8, 48, 40), 2, 6, SEEDS[1]
    c = fresh(blob_of("box_edge"))
    try:
        with c.progressive(region, spp, spp_max=spp_max, seed=seed) as prog:
            last = None
            for target in (2, 6):
                prog.advance(target)
                ns = prog.read()[2]
                dev = prog.ao_device(K, EDGE_RADIUS)
                c.synchronize()
                dev = planes_numpy(dev)
                want = device_planes(c, region, spp_max, K, EDGE_RADIUS, ns=torch.from_numpy(ns.view(np.int32)).cuda(), seed=seed)
                assert not differing(dev, want), target
                assert dev["rays"].max() == K * int(ns.max()) and (dev["open"] > 0).any() and (dev["open"] < dev["rays"]).any()
                other_seed = device_planes(c, region, spp_max, K, EDGE_RADIUS, ns=torch.from_numpy(ns.view(np.int32)).cuda(), seed=seed + 1)
                assert not np.array_equal(other_seed["open"], dev["open"])
                assert last is None or not np.array_equal(last, dev["rays"])
                last = dev["rays"]
                print("progressive: target", target, "counts", np.unique(ns).tolist())
    finally:
        c.close()


def test_points_are_the_regions_rays_and_follow_a_permutation(frames):
    import torch
    from qaray_amd import hip
    c = fresh(blob_of("box_edge"))
    try:
        radius = EDGE_RADIUS
        hits = first_hits(c, REGION, 0, 1)
        hit = hits["hit"][..., 0]
        pts, nrm = hits["point"][..., 0, :][hit], hits["normal"][..., 0, :][hit]
        ids = stream_ids(REGION, W)[hit].astype(np.uint32).view(np.int32)
        region = device_planes(c, REGION, 1, K, radius, first=0)
        dev = torch.device("cuda", 0)
        tp, tn, ti = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (pts, nrm, ids))
        got = c.ao_points_device(tp, tn, K, radius, first=0, stream_ids=ti)
        c.synchronize()
        open_ = got["open"].cpu().numpy().view(np.uint32)
        assert hit.any() and not hit.all()
        assert np.array_equal(open_, region["open"][hit]) and (open_ > 0).any() and (open_ < K).any()
        assert np.array_equal(bits(got["ao"].cpu().numpy()), bits(ao_ref(open_, np.full(len(open_), K))))
        host = c.ao_points(pts, nrm, K, radius, first=0, stream_ids=ids)
        assert np.array_equal(host["open"], open_) and np.array_equal(bits(host["ao"]), bits(got["ao"].cpu().numpy()))
        # a fixed permutation of the points gives the permuted result
        perm = np.random.default_rng(11).permutation(len(pts))
        tperm = torch.from_numpy(perm).to(dev)
        again = c.ao_points_device(tp[tperm].contiguous(), tn[tperm].contiguous(), K, radius, stream_ids=ti[tperm].contiguous())
        c.synchronize()
        assert np.array_equal(again["open"].cpu().numpy().view(np.uint32), open_[perm])
        # without stream ids the stream is the point's index: the ids spelled out give the same
        plain = c.ao_points(pts, nrm, 8, radius, first=5)
        spelled = c.ao_points(pts, nrm, 8, radius, first=5, stream_ids=np.arange(len(pts)))
        assert np.array_equal(plain["open"], spelled["open"]) and not np.array_equal(plain["open"], c.ao_points(pts, nrm, 8, radius, first=6)["open"])
        # void points: NaN and the infinities in each of the six components, and a zero normal
        vp, vn = [], []
        for bad in (np.nan, np.inf, -np.inf):
            for k in range(6):
                rec = np.float32([0.0, -10.0, 11.0, 0.0, 0.6, 0.8])
                rec[k] = bad
                vp.append(rec[:3])
                vn.append(rec[3:])
        vp.append(np.float32([0.0, -10.0, 11.0]))
        vn.append(np.float32([0.0, 0.0, 0.0]))
        void = c.ao_points(np.float32(vp), np.float32(vn), 7, 5.0)
        assert len(vp) == 19 and (void["open"] == 7).all() and (void["ao"] == 1).all()
        # n = 0 answers without a launch
        empty = c.ao_points(np.zeros((0, 3), F32), np.zeros((0, 3), F32))
        assert empty["open"].shape == (0,)
        assert hip.lib().qa_ao_points_device(c._h, 0, None, None, None, 0, K, 5.0, 1, None, None, None) == 0
    finally:
        c.close()


def test_refusals_write_nothing():
    import torch
    from qaray_amd import hip
    L = hip.lib()
    region = (5, 3, 45, 27)
    h, w = region[3] - region[1], region[2] - region[0]
    nan = float("nan")

    def sentinels():
        return {"open": torch.full((h, w), 7, dtype=torch.int32, device="cuda:0"), "rays": torch.full((h, w), 7, dtype=torch.int32, device="cuda:0"),
                "ao": torch.full((h, w), 7.0, dtype=torch.float32, device="cuda:0")}

    def untouched(t):
        torch.cuda.synchronize()
        return all(bool((v == 7).all()) for v in t.values())

    c = fresh(blob_of("box"))
    try:
        t = sentinels()
        ptr = [t[k].data_ptr() for k in hip.AO_PLANES]
        call = lambda reg=region, first=0, spp=4, k=K, radius=5.0, planes=ptr: L.qa_ao_region_device(c._h, *reg, first, spp, None, k, radius, 1, *planes, None)   # noqa: E731
        assert call() == 0
        c.synchronize()
        assert not untouched(t)
        t = sentinels()
        ptr = [t[k].data_ptr() for k in hip.AO_PLANES]
        assert call(planes=ptr, k=0) == QA_EINVAL and call(planes=ptr, k=257) == QA_EINVAL
        assert call(planes=ptr, k=256, spp=2, radius=0.02) == 0      # the largest K is taken
        c.synchronize()
        t = sentinels()
        ptr = [t[k].data_ptr() for k in hip.AO_PLANES]
        assert call(planes=ptr, spp=0) == QA_EINVAL
        assert call(planes=ptr, first=2 ** 30 - 2, spp=4, k=4) == QA_EINVAL           # (first + spp) * K = 2^32 + 8
        assert call(planes=ptr, first=2 ** 31, spp=4) == QA_EINVAL
        for radius in (nan, 0.0, -1.0, float(QA_BIAS), -INF):
            assert call(planes=ptr, radius=radius) == QA_EINVAL, radius
        assert call(planes=[None, None, None]) == QA_EINVAL                              # no plane
        for bad in ((5, 3, 5, 27), (-1, 0, 10, 10), (0, 0, SIZE[0] + 1, 10)):
            assert call(reg=bad, planes=ptr) == QA_EINVAL, bad
        assert L.qa_ao_region(c._h, *region, 0, 4, None, 0, 5.0, 1, None, None, None) == QA_EINVAL
        # the points form: K, radius, first + K, the ray queries' rules for n
        o = torch.zeros((8, 3), device="cuda:0")
        nn = torch.tensor([[0.0, 0.0, 1.0]] * 8, device="cuda:0")
        po, pn, pout = o.data_ptr(), nn.data_ptr(), t["open"].data_ptr()
        points = lambda n=8, first=0, k=K, radius=5.0, a=po, b=pn, out=pout: L.qa_ao_points_device(c._h, n, a, b, None, first, k, radius, 1, out, None, None)   # noqa: E731
        assert points(k=0) == QA_EINVAL and points(k=257) == QA_EINVAL and points(radius=nan) == QA_EINVAL and points(radius=0.005) == QA_EINVAL
        assert points(first=2 ** 32 - 3, k=4) == QA_EINVAL and points(first=2 ** 32 - 4, k=4) == 0
        c.synchronize()
        t = sentinels()
        pout = t["open"].data_ptr()
        assert points(n=2 ** 31, out=pout) == QA_EINVAL and points(a=None, out=pout) == QA_EINVAL and points(out=None) == QA_EINVAL
        assert L.qa_ao_points(c._h, 8, None, None, None, 0, K, 5.0, 1, None, None) == QA_EINVAL
        assert untouched(t)
        # Python: raised before the library is reached
        with pytest.raises(TypeError):
            c.ao_device(region, 4, open=torch.zeros((h, w), dtype=torch.float32, device="cuda:0"))     # dtype
        with pytest.raises(ValueError):
            c.ao_device(region, 4, ao=torch.zeros((h, w + 1), device="cuda:0"))                         # shape
        with pytest.raises(ValueError):
            c.ao_device(region, 4, ao=torch.zeros((h, w)))                                              # device
        with pytest.raises(ValueError):
            c.ao_device(region, 4, ao=torch.zeros((w, h), device="cuda:0").t())                         # contiguity
        with pytest.raises(TypeError):
            c.ao_device(region, 4, ao=np.zeros((h, w), F32))
        with pytest.raises(TypeError):
            c.ao_points_device(np.zeros((8, 3), F32), nn)
        with pytest.raises(TypeError):
            c.ao_points_device(o.double(), nn)
        with pytest.raises(ValueError):
            c.ao_points_device(o, nn[:7])
        with pytest.raises(ValueError):
            c.ao_points_device(o.cpu(), nn)
        with pytest.raises(ValueError):
            c.ao_points_device(torch.zeros((3, 8), device="cuda:0").t(), nn)
        with pytest.raises(TypeError):
            c.ao_points_device(o, nn, stream_ids=torch.zeros(8, device="cuda:0"))
        with pytest.raises(ValueError):
            c.ao(region, 4, ns=np.zeros((h, w + 1), np.uint32))
        with pytest.raises(ValueError):
            c.ao_points(np.zeros((8, 3)), np.zeros((7, 3)))
    finally:
        c.close()
    # no scene
    bare = hip.Context(0)
    try:
        t = sentinels()
        ptr = [t[k].data_ptr() for k in hip.AO_PLANES]
        assert L.qa_ao_region_device(bare._h, *region, 0, 4, None, K, 5.0, 1, *ptr, None) == QA_ENOSCENE
        assert L.qa_ao_points_device(bare._h, 0, None, None, None, 0, K, 5.0, 1, None, None, None) == QA_ENOSCENE
        assert untouched(t)
    finally:
        bare.close()
    # a camera with depth of field: the region and progressive forms are refused, the points form answers
    d = fresh(dof_blob())
    try:
        t = sentinels()
        with pytest.raises(hip.HipError) as e:
            d.ao_device(region, 4, **t)
        assert e.value.code == QA_EUNSUPPORTED and "depth of field" in str(e.value)
        with pytest.raises(hip.HipError) as e:
            d.ao(region, 4)
        assert e.value.code == QA_EUNSUPPORTED
        with d.progressive(region, 2) as prog:
            prog.advance(1)
            with pytest.raises(hip.HipError) as e:
                prog.ao_device(**t)
            assert e.value.code == QA_EUNSUPPORTED
        d.synchronize()
        assert untouched(t)
        pts = d.ao_points(np.float32([[0, 0, 0.01], [0, 0, 5]]), np.float32([[0, 0, 1], [0, 0, 1]]), 16, 50.0)
        assert pts["open"].shape == (2,) and (pts["open"] <= 16).all()
    finally:
        d.close()
    # the progressive form without a frame
    c = fresh(blob_of("box"))
    try:
        t = sentinels()
        assert L.qa_progressive_ao_device(c._h, K, 5.0, *(t[k].data_ptr() for k in hip.AO_PLANES), None) == QA_EINVAL
        assert untouched(t)
    finally:
        c.close()


def test_nothing_else_moves_and_two_runs_agree(frames):
    c = fresh(blob_of("teapot"))
    try:
        radius = frames["teapot"]["radii"][1]
        frame0 = c.render_region(REGION, 2, seed=SEEDS[0])
        cnt0, time0 = c.counters(), c.kernel_time()
        first = device_planes(c, REGION, SPP, K, radius)
        hits = frames["teapot"]["hits", "region", 0]
        pts, nrm = hits["point"][hits["hit"]], hits["normal"][hits["hit"]]
        p0 = c.ao_points(pts, nrm, 8, radius)
        for _ in range(2):
            again = device_planes(c, REGION, SPP, K, radius)
            assert not differing(first, again)
            c.ao(RAGGED, 2, 16, INF, first=1)
            p1 = c.ao_points(pts, nrm, 8, radius)
            assert np.array_equal(p0["open"], p1["open"]) and np.array_equal(bits(p0["ao"]), bits(p1["ao"]))
        assert not differing(first, frames["teapot"]["got", "region", 0, 1])
        assert c.counters() == cnt0 and c.kernel_time() == time0
        frame1 = c.render_region(REGION, 2, seed=SEEDS[0])
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(frame0, frame1))
    finally:
        c.close()
