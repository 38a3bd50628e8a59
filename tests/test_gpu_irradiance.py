"""Irradiance queries (qa_irradiance.hip: qa_irradiance_points*; the unit's opening comment is the specification).  The anchor: on a
surface whose material is the white diffuse record, the light at the points cast_rays reports is bit for bit the radiance of the rays
that hit them - which ties the call to qa_radiance_rays, and through its own anchor to every frame test there is.  The rest checks what
the specification says of points: independence of batch and order, closed forms, void points, state and refusals.

Radiance and point calls only: no frame of an area-light scene is rendered here."""
import ctypes as C

import numpy as np
import pytest

from gbuffer_util import REGION, SEEDS, bits, scene_blob
from radiance_util import AREA_BOX, QA_EINVAL, QA_ENOSCENE, QA_EUNSUPPORTED, QA_LIGHT_POINT, SOFTSHADOW, anchor_blob, variant
from ray_query_util import BOX, fresh, void_rays

pytestmark = pytest.mark.gpu

# no committed scene file has textures, point lights of no size, an LDS-resident image and a material without texmaps that the camera
# sees: example_project10_objects.xml with its area lights shrunk to points reaches that instance, <RES=1,LIGHTS=1,TEX=1,AREA=0>
POINT_LIT_OBJECTS = "example_project10_objects.xml with point lights"
# the smallest set that reaches the ten instances, one scene each: scene -> (RES, LIGHTS, TEX, AREA)
ANCHOR = {
    "example_project11_teapot.xml": (0, 0, 0, 0),
    "example_project11_box.xml": (0, 1, 0, 0),
    "example_project7_checkboard.xml": (0, 1, 1, 0),
    AREA_BOX: (0, 1, 0, 1),
    "example_project10_test.xml": (0, 1, 1, 1),
    BOX: (1, 0, 0, 0),
    "example_project3_sphere.xml": (1, 1, 0, 0),
    POINT_LIT_OBJECTS: (1, 1, 1, 0),
    SOFTSHADOW: (1, 1, 0, 1),
    "example_project10_objects.xml": (1, 1, 1, 1),
}
LIT_BOX = "example_project3_box.xml"
ONE_LIGHT = "example_project11_box.xml"
COLOURS = ("diffuse", "specular", "reflection", "refraction", "emission")


def blob_of(scene):
    if scene == POINT_LIT_OBJECTS:
        from qaray_amd import hip
        blob = scene_blob("example_project10_objects.xml").copy()
        lights = hip.blob_table(blob, "lights")
        assert (lights["size"] > 0.01).any()
        lights["size"] = 0
        return blob
    return anchor_blob(scene)


def white(record):
    """The record of the specification in a material's place: diffuse (1, 1, 1), everything else 0; texmap references stay (none)"""
    rec = record.copy()
    for f in COLOURS:
        rec[f]["color"] = 1.0 if f == "diffuse" else 0.0
    for f in ("absorption", "kill", "gloss_spec", "gloss_refl", "gloss_refr"):
        rec[f] = 0
    return rec


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def first_hits(c):
    """The region's camera rays and their closest hits -> (origins, dirs, cast) numpy"""
    o, d = c.camera_rays(REGION, SEEDS[0])
    return o, d, c.cast_rays(o, d)


def facing_points(c, n=None):
    """Points on the surfaces the camera sees, normals turned towards the camera; misses left out -> (points, normals) float32"""
    o, d, cast = first_hits(c)
    hit = cast["ids"][:, 0] >= 0
    p, nr = cast["point"][hit], cast["normal"][hit]
    nr = (nr * -np.sign((nr * d[hit]).sum(axis=1, keepdims=True))).astype(np.float32)
    keep = (nr != 0).any(axis=1)
    return p[keep][:n], nr[keep][:n]


@pytest.mark.parametrize("scene", list(ANCHOR))
def test_the_light_at_a_white_surface_is_the_radiance_of_the_rays_that_hit_it(scene):
    """The anchor, bit for bit.  Among the materials without texmaps that the region's camera rays hit on front faces, the one hit
    most is set to the white record; for the rays that hit it, irradiance_points_device at cast_rays' point and normal equals
    radiance_rays_device of the rays (miss_environment) in rgb and ns, with the pixel's stream id, at spp 1 and 3 and max_bounce 0
    and 5.  The scene runs the instance the table names."""
    from qaray_amd import hip
    blob = blob_of(scene)
    c = fresh(blob)
    try:
        assert variant(c.kernel_name()) == ANCHOR[scene], scene
        o, d, cast = first_hits(c)
        mats = hip.blob_table(blob, "materials")
        word = cast["ids"][:, 1]
        front = (cast["ids"][:, 0] >= 0) & (word >= 0) & (word < hip.QA_GBUFFER_BACKFACE)
        plain = np.array([all(int(m[f]["texmap"]) < 0 for f in COLOURS) for m in mats])
        count = np.bincount(word[front], minlength=len(mats)) * plain
        m = int(count.argmax())
        assert count[m] >= 150, (scene, count)
        c.edit_materials(m, white(mats[m:m + 1]))
        assert variant(c.kernel_name()) == ANCHOR[scene], "the edit keeps the instance"
        sel = front & (word == m)
        sid = dev(np.flatnonzero(sel).astype(np.int32))
        to, td, tp, tn = dev(o[sel]), dev(d[sel]), dev(cast["point"][sel]), dev(cast["normal"][sel])
        lit = False
        for spp, seed in ((1, SEEDS[0]), (3, SEEDS[1])):
            for max_bounce in (0, 5):
                want = c.radiance_rays_device(to, td, spp, max_bounce, seed, stream_ids=sid, miss_environment=True)
                got = c.irradiance_points_device(tp, tn, spp, max_bounce, seed, stream_ids=sid)
                c.synchronize()
                rgb, ns = got[0].cpu().numpy(), got[1].cpu().numpy()
                w_rgb, w_ns = want[0].cpu().numpy(), want[2].cpu().numpy()
                assert np.array_equal(ns, w_ns) and (ns == spp).all(), (scene, spp, max_bounce)
                differ = (bits(rgb) != bits(w_rgb)).any(axis=1)
                assert not differ.any(), (scene, spp, max_bounce, int(differ.sum()), int(sel.sum()))
                lit = lit or bool((rgb > 0).any())
        assert lit, "some light arrives somewhere"
    finally:
        c.close()


def test_the_anchor_reaches_all_ten_instances():
    """By the accounting of tests/test_gpu_radiance.py: the five shadings of PickShading, in LDS and in global memory (the anchor
    asserts each scene's instance against kernel_name())"""
    shadings = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 0, 1), (1, 1, 1)]
    assert set(ANCHOR.values()) == {(res,) + s for res in (0, 1) for s in shadings} and len(ANCHOR) == 10


def test_a_points_answer_depends_on_point_stream_seed_and_spp_alone():
    """Batches of 1, 63, 64, 65 and 130 points - below, at and above a work item's 64, and more than one item - give per-point
    results equal to the largest batch's, and a permutation with its stream ids gives the permuted results, bit for bit."""
    rng = np.random.default_rng(20251021)
    c = fresh(scene_blob(LIT_BOX))
    try:
        p, nr = facing_points(c)
        pick = rng.choice(len(p), 130, replace=False)
        p, nr = p[pick], nr[pick]
        ids = rng.integers(0, 1 << 20, 130).astype(np.uint32)
        whole = c.irradiance_points(p, nr, spp=2, max_bounce=3, seed=SEEDS[1], stream_ids=ids)
        assert (whole[1] == 2).all() and (whole[0] > 0).any() and len(np.unique(whole[0], axis=0)) > 100
        for n in (1, 63, 64, 65, 130):
            part = c.irradiance_points(p[:n], nr[:n], spp=2, max_bounce=3, seed=SEEDS[1], stream_ids=ids[:n])
            perm = rng.permutation(n)
            shuffled = c.irradiance_points(p[:n][perm], nr[:n][perm], spp=2, max_bounce=3, seed=SEEDS[1], stream_ids=ids[:n][perm])
            for a, b, w in zip(part, shuffled, whole):
                assert np.array_equal(bits(a), bits(w[:n])), n
                assert np.array_equal(bits(b), bits(w[:n][perm])), n
        # without stream ids a point's stream is its index: the same as ids 0 .. n - 1
        a = c.irradiance_points(p[:65], nr[:65], spp=2)
        b = c.irradiance_points(p[:65], nr[:65], spp=2, stream_ids=np.arange(65))
        assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))
        # and each of the other arguments matters
        for kw in (dict(seed=SEEDS[0]), dict(spp=3), dict(max_bounce=0), dict(stream_ids=ids[::-1].copy())):
            other = c.irradiance_points(p, nr, **{**dict(spp=2, max_bounce=3, seed=SEEDS[1], stream_ids=ids), **kw})
            assert not np.array_equal(bits(other[0]), bits(whole[0])), kw
    finally:
        c.close()


def test_closed_forms_on_the_unlit_box_and_under_one_point_light():
    """The Cornell box has no lights and spans x, y in [-13.9, 13.9], z in [-3, 25].  A point outside it that faces away sees the
    environment alone: exactly its colour at any spp (every sample is 1 * c, and the mean of a constant is exact); with max_bounce 0
    nothing is spawned and nothing lights the point: exactly 0.  Under one point light, a point that faces away from it has
    cosNL = 0: exactly 0 at max_bounce 0."""
    from qaray_amd import hip
    blob = scene_blob(BOX)
    colour = np.float32([0.75, 0.0625, 0.375])
    c = fresh(blob)
    try:
        env = hip.blob_backdrop(blob)[1].copy()
        assert int(env["texmap"]) < 0
        env["color"] = colour
        c.edit_backdrop(environment=env)
        p = np.float32([[0, 0, 40], [30, 0, 10], [-30, 2, 10], [0, 40, 10], [1, -40, 10], [0, 0, -20], [25, 25, 30]])
        nr = np.float32([[0, 0, 1], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, -1], [0.6, 0, 0.8]])
        for spp in (1, 4, 7):
            rgb, ns = c.irradiance_points(p, nr, spp=spp)
            assert (ns == spp).all() and np.array_equal(bits(rgb), bits(np.broadcast_to(colour, rgb.shape))), spp
        q, qn = facing_points(c, 200)
        assert len(q) == 200
        rgb, ns = c.irradiance_points(q, qn, spp=3, max_bounce=0)
        assert (ns == 3).all() and not bits(rgb).any()
        assert (c.irradiance_points(q, qn, spp=3, max_bounce=2)[0] > 0).any()   # (with bounces the emitter and the environment arrive)
    finally:
        c.close()
    blob = scene_blob(ONE_LIGHT)
    lights = hip.blob_table(blob, "lights")
    lit = lights[lights["type"] != 0]
    assert len(lit) == 1 and int(lit[0]["type"]) == QA_LIGHT_POINT
    c = fresh(blob)
    try:
        q, _ = facing_points(c, 300)
        away = q - lit[0]["position"]
        away = (away / np.linalg.norm(away, axis=1, keepdims=True)).astype(np.float32)
        rgb, ns = c.irradiance_points(q, away, spp=2, max_bounce=0)
        assert (ns == 2).all() and not bits(rgb).any()
        assert (c.irradiance_points(q, -away, spp=2, max_bounce=0)[0] > 0).any()   # (towards it: where nothing is in the way, light)
    finally:
        c.close()


def test_void_points_are_black_samples_that_disturb_nothing():
    """NaN and both infinities in each of the six components, and a zero normal, spread among good points: rgb 0, ns spp; the good
    points keep their bits."""
    c = fresh(scene_blob(LIT_BOX))
    try:
        gp, gn = facing_points(c, 150)
        vp, vn = void_rays()
        at = np.linspace(0, len(gp), len(vp), dtype=int)
        p, nr = np.insert(gp, at, vp, axis=0), np.insert(gn, at, vn, axis=0)
        void = ~(np.isfinite(p).all(axis=1) & np.isfinite(nr).all(axis=1)) | (nr == 0).all(axis=1)
        assert void.sum() == 19
        ids = np.zeros(len(p), np.uint32)
        ids[~void] = np.arange(len(gp))
        ids[void] = 7
        alone = c.irradiance_points(gp, gn, spp=3, stream_ids=np.arange(len(gp)))
        rgb, ns = c.irradiance_points(p, nr, spp=3, stream_ids=ids)
        assert not bits(rgb[void]).any() and (ns == 3).all()
        assert np.array_equal(bits(rgb[~void]), bits(alone[0])) and (alone[0] > 0).any()
    finally:
        c.close()


def test_state_counters_and_refusals():
    """A frame has the same bits before and after a call; the counters move by n * spp samples and the kernel time by one launch;
    every refusal of the C ABI leaves the outputs alone; Python's argument errors are raised before the library is entered."""
    import torch
    from qaray_amd import hip
    L = hip.lib()
    c = fresh(scene_blob(LIT_BOX))
    try:
        p, nr = facing_points(c, 200)
        n = len(p)
        frame0 = c.render_region(REGION, 2, seed=SEEDS[0])
        name = c.kernel_name()
        c.reset_counters()
        launches0 = c.kernel_time()[1]
        c.irradiance_points(p, nr, spp=3, max_bounce=0)
        cnt = c.counters()
        assert cnt["samples"] == 3 * n and cnt["casts_normal"] == 0 and c.kernel_time()[1] == launches0 + 1 and c.kernel_name() == name
        c.reset_counters()
        c.irradiance_points(p, nr, spp=3, max_bounce=1)
        cnt = c.counters()
        assert cnt["samples"] == 3 * n and 0 < cnt["casts_normal"] <= 3 * n   # (one bounce ray per sample that spawns, none to reach the point)
        frame1 = c.render_region(REGION, 2, seed=SEEDS[0])
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(frame0, frame1))

        n = 64
        tp, tn = dev(p[:n]), dev(nr[:n])
        rgb = torch.full((n, 3), 7.0, device="cuda:0")
        ns = torch.full((n,), 7, dtype=torch.int32, device="cuda:0")
        pp_, pn_, prgb, pns = (x.data_ptr() for x in (tp, tn, rgb, ns))
        par = hip.RadianceParams.default()
        pp = C.byref(par)
        device = lambda h, n, *a: L.qa_irradiance_points_device(h, n, *a, None)   # noqa: E731
        hrgb = np.full((n, 3), 7, np.float32)
        hp, hn = p[:n].ctypes.data, nr[:n].ctypes.data
        # n == 0 launches nothing and needs no array
        assert device(c._h, 0, None, None, None, None, None, None) == 0
        assert L.qa_irradiance_points(c._h, 0, None, None, None, None, None, None) == 0
        assert c.irradiance_points(np.zeros((0, 3)), np.zeros((0, 3)))[0].shape == (0, 3)
        refused = [
            (1 << 31, pp_, pn_, None, pp, prgb, pns),    # n beyond 2^31 - 1 (nothing is sized by it)
            (1 << 40, pp_, pn_, None, pp, prgb, pns),
            (n, None, pn_, None, pp, prgb, pns),         # a null point or normal array
            (n, pp_, None, None, pp, prgb, pns),
            (n, pp_, pn_, None, pp, None, pns),          # a null rgb
            (n, pp_, pn_, None, None, prgb, pns),        # null params
        ]
        for args in refused:
            assert device(c._h, *args) == QA_EINVAL, args
        for field, bad in (("spp", 0), ("spp", -3), ("max_bounce", -1), ("flags", 1), ("flags", 2), ("flags", 4)):
            q = hip.RadianceParams.default()
            setattr(q, field, bad)
            assert device(c._h, n, pp_, pn_, None, C.byref(q), prgb, pns) == QA_EINVAL, field
            assert L.qa_irradiance_points(c._h, n, hp, hn, None, C.byref(q), hrgb.ctypes.data, None) == QA_EINVAL
        assert L.qa_irradiance_points(c._h, 1 << 31, hp, hn, None, pp, hrgb.ctypes.data, None) == QA_EINVAL
        assert L.qa_irradiance_points(c._h, n, hp, None, None, pp, hrgb.ctypes.data, None) == QA_EINVAL
        assert L.qa_irradiance_points(c._h, n, hp, hn, None, pp, None, None) == QA_EINVAL
        assert device(None, n, pp_, pn_, None, pp, prgb, pns) == QA_EINVAL
        bare = hip.Context(0)
        try:
            assert device(bare._h, n, pp_, pn_, None, pp, prgb, pns) == QA_ENOSCENE
            assert L.qa_irradiance_points(bare._h, n, hp, hn, None, pp, hrgb.ctypes.data, None) == QA_ENOSCENE
        finally:
            bare.close()
        c.synchronize()
        torch.cuda.synchronize()
        assert (rgb == 7.0).all() and (ns == 7).all() and (hrgb == 7).all()   # a refusal writes nothing
        # optional output: rgb alone
        assert device(c._h, n, pp_, pn_, None, pp, prgb, None) == 0
        c.synchronize()
        want = c.irradiance_points(p[:n], nr[:n], spp=par.spp)
        assert np.array_equal(bits(rgb.cpu().numpy()), bits(want[0])) and (ns == 7).all()
        # on a stream of the caller's, into tensors of the caller's
        s = torch.cuda.Stream(device="cuda:0")
        with torch.cuda.stream(s):
            sp, sn = dev(p[:n]), dev(nr[:n])
            got = c.irradiance_points_device(sp, sn, spp=par.spp, rgb=rgb, ns=ns, stream=s.cuda_stream)
        s.synchronize()
        assert got[0] is rgb and got[1] is ns and all(np.array_equal(bits(a.cpu().numpy()), bits(b)) for a, b in zip(got, want))

        # Python: raised before the library is reached
        with pytest.raises(TypeError):
            c.irradiance_points_device(p[:n], nr[:n])                        # numpy where a tensor is expected
        with pytest.raises(TypeError):
            c.irradiance_points_device(tp.double(), tn)                      # dtype
        with pytest.raises(TypeError):
            c.irradiance_points_device(tp, tn, ns=torch.empty(n, device="cuda:0"))
        with pytest.raises(TypeError):
            c.irradiance_points_device(tp, tn, stream_ids=torch.zeros(n, device="cuda:0"))
        with pytest.raises(ValueError):
            c.irradiance_points_device(tp.cpu(), tn)                         # device
        with pytest.raises(ValueError):
            c.irradiance_points_device(tp, tn[:n - 1])                       # shape
        with pytest.raises(ValueError):
            c.irradiance_points_device(tp, tn, rgb=torch.empty((n, 4), device="cuda:0"))
        with pytest.raises(ValueError):
            c.irradiance_points_device(torch.empty((n, 6), device="cuda:0")[:, :3], tn)   # contiguity
        with pytest.raises(ValueError):
            c.irradiance_points(p[:n], nr[:n - 1])
        with pytest.raises(ValueError):
            c.irradiance_points(p[:n], nr[:n], stream_ids=np.arange(n + 1))
    finally:
        c.close()


def test_photon_maps_and_long_area_light_paths_are_refused():
    """With photon maps built the call is refused (no gathering instance is compiled) and accepted again once they are cleared; area
    lights with max_bounce > 7 are refused as a frame refuses them.  Both refusals leave the outputs unwritten."""
    import torch
    from qaray_amd import hip
    c = fresh(scene_blob("custom_photon.xml"))
    try:
        p, nr = facing_points(c, 100)
        tp, tn = dev(p), dev(nr)
        rgb = torch.full((len(p), 3), 7.0, device="cuda:0")
        c.build_photon_maps((3000, 20, 0.2), (400, 20, 1.0))
        with pytest.raises(hip.HipError) as e:
            c.irradiance_points_device(tp, tn, rgb=rgb)
        assert e.value.code == QA_EUNSUPPORTED
        c.synchronize()
        assert (rgb == 7.0).all()
        c.clear_photon_maps()
        out, ns = c.irradiance_points(p, nr, spp=2)
        assert (ns == 2).all() and (out > 0).any()
    finally:
        c.close()
    c = fresh(anchor_blob(SOFTSHADOW))
    try:
        assert variant(c.kernel_name())[3] == 1
        p, nr = facing_points(c, 100)
        tp, tn = dev(p), dev(nr)
        rgb = torch.full((len(p), 3), 7.0, device="cuda:0")
        with pytest.raises(hip.HipError) as e:
            c.irradiance_points_device(tp, tn, max_bounce=8, rgb=rgb)
        assert e.value.code == QA_EUNSUPPORTED
        c.synchronize()
        assert (rgb == 7.0).all()
        assert (c.irradiance_points(p, nr, spp=1, max_bounce=7)[1] == 1).all()
    finally:
        c.close()
