"""The id matte (qa_idmatte_region*, qa_progressive_idmatte_device, qa_idmatte_select_device: qa_idmatte.hip) against an independent
route: the camera rays of every sample handed out (camera_sample_rays_device), cast as rays of the caller's (cast_rays_device) - both
pinned to the CPU oracle by their own tests - and the numpy restatement of qa_idmatte_dev.h's opening comment (idmatte_util) over the
ids that come back.  Every comparison of ids, counts, other and samples is exact.

Scenes, in frames of 64x48: the Cornell box (the LDS-resident kernel), a 40x24 region over the light's edge and the boxes' silhouettes
at 16 spp; custom_textures.xml (the textured kernel), 32x24 over the spheres' and the mesh's silhouettes at 8 spp;
example_project7_object.xml (meshes in global memory), 24x16 over the teapot's, the dolls' and the monkey's silhouettes at 8 spp.  Each
case asserts that some pixel of the computed result holds two or more ids, under both keys."""
import functools
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from idmatte_util import EMPTY, F32, KEYS, MISS, SLOTS, key_of, occupied, route, route_planes, same_planes, select_ref
from matte_util import linear_byte

pytestmark = pytest.mark.gpu
QA_EINVAL = -1
QA_EUNSUPPORTED = -6
SIZE = (64, 48)
BOX, TEXTURES, OBJECTS = "example_project12_box.xml", "custom_textures.xml", "example_project7_object.xml"
GRID = os.path.join(GOLDEN, "idmatte", "grid.xml")
DOF_SCENE = "custom_softshadow.xml"
# scene -> (region, spp, the <RES, TEX> it must reach; None: whichever)
CASES = {BOX: ((12, 3, 52, 27), 16, ("RES=1", "TEX=0")), TEXTURES: ((16, 10, 48, 34), 8, ("TEX=1",)), OBJECTS: ((18, 12, 42, 28), 8, ("RES=0",))}


@functools.lru_cache(maxsize=None)
def blob_of(scene, size=SIZE):
    from gbuffer_util import scene_blob
    return scene_blob(scene, size)


def fresh(blob):
    from qaray_amd import hip
    c = hip.Context(0)
    c.set_option("coop", 0)   # (kernel_name() then names qa_integrate<RES=..,TEX=..> for every scene)
    c.upload_scene(blob)
    return c


def host(planes):
    return {k: v.cpu().numpy() for k, v in planes.items()}


@pytest.fixture(scope="module")
def cases():
    """scene -> dict: "route" -> (hit, ids2) of the region at the case's spp; key -> the four planes (host variant) at that spp;
    ("one", key) -> the planes at 1 spp; "gbuffer" -> the first-hit planes; "coverage" -> matte's coverage at the case's spp; "name" -> the kernel's"""
    out = {}
    for scene, (region, spp, _) in CASES.items():
        c = fresh(blob_of(scene))
        try:
            d = {"route": route(c, region, spp), "gbuffer": c.gbuffer(region), "coverage": c.matte(region, spp)["coverage"], "name": c.kernel_name()}
            for key in KEYS:
                d[key] = c.idmatte(region, spp, key)
                d["one", key] = c.idmatte(region, 1, key)
            out[scene] = d
        finally:
            c.close()
    return out


@pytest.mark.parametrize("scene", list(CASES))
def test_the_scenes_reach_their_kernels(cases, scene):
    assert all(tag in cases[scene]["name"] for tag in CASES[scene][2]), cases[scene]["name"]


@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("scene", list(CASES))
def test_one_sample_is_the_first_hit_ids(cases, scene, key):
    m, g = cases[scene]["one", key], cases[scene]["gbuffer"]
    hit = g["depth"] != MISS
    assert hit.any()
    assert np.array_equal(m["ids"][..., 0][hit], key_of(g["ids"], key)[hit]) and (m["counts"][..., 0][hit] == 1).all()
    assert (m["ids"][..., 0][~hit] == EMPTY).all() and not m["counts"][..., 0][~hit].any()
    assert (m["ids"][..., 1:] == EMPTY).all() and not m["counts"][..., 1:].any() and not m["other"].any() and (m["samples"] == 1).all()


@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("scene", list(CASES))
def test_the_planes_are_the_ray_queries_ids_tabled(cases, scene, key):
    got = cases[scene][key]
    most = int(occupied(got).max())
    print(scene, key, "most ids in a pixel:", most, "pixels with two or more:", int((occupied(got) >= 2).sum()))
    assert most >= 2, "the crop shows no pixel with two ids: the comparison would pass on one-id pixels alone"
    want = route_planes(*cases[scene]["route"], key)
    assert not same_planes(got, want), (scene, key, same_planes(got, want))
    assert (got["samples"] == CASES[scene][1]).all()


@pytest.mark.parametrize("scene", list(CASES))
def test_the_counts_sum_to_the_matte_planes_coverage(cases, scene):
    for key in KEYS:
        m = cases[scene][key]
        hits = m["counts"].sum(axis=-1, dtype=np.uint32) + m["other"]
        cov = hits.astype(F32) / m["samples"].astype(F32)
        assert np.array_equal(cov.view(np.uint32), cases[scene]["coverage"].view(np.uint32)), key


def test_an_ns_plane_gives_each_pixel_its_own_count(cases):
    import torch
    region, spp, _ = CASES[OBJECTS]
    h, w = region[3] - region[1], region[2] - region[0]
    hit, ids2 = cases[OBJECTS]["route"]
    syn = np.random.default_rng(5).choice(np.array([0, 1, 3, spp, spp + 5, 2 ** 31, 2 ** 32 - 1], np.uint32), size=(h, w))
    n = np.minimum(syn, spp)
    c = fresh(blob_of(OBJECTS))
    try:
        for key in KEYS:
            got = c.idmatte(region, spp, key, ns=syn)
            assert not same_planes(got, route_planes(hit, ids2, key, n)), key
            assert np.array_equal(got["samples"], n)
            zero = syn == 0
            assert zero.any() and (got["ids"][zero] == EMPTY).all() and not got["counts"][zero].any() and not got["other"][zero].any()
            dev = c.idmatte_device(region, spp, key, ns=torch.from_numpy(syn.view(np.int32)).cuda())
            c.synchronize()
            assert not same_planes(host(dev), got), key
    finally:
        c.close()


@pytest.mark.parametrize("scene", [BOX, OBJECTS])
def test_a_ragged_region_off_the_tile_grid_is_the_aligned_calls_block(cases, scene):
    region, spp, _ = CASES[scene]
    x0, y0 = region[0] + 5, region[1] + 3          # neither a multiple of 8, nor is the region's origin plus it
    sub = (x0, y0, x0 + 13, y0 + 11)
    assert x0 % 8 and y0 % 8
    c = fresh(blob_of(scene))
    try:
        for key in KEYS:
            got = c.idmatte(sub, spp, key)
            want = {k: v[3:14, 5:18] for k, v in cases[scene][key].items()}
            assert got["ids"].shape == (11, 13, SLOTS) and not same_planes(got, want), key
    finally:
        c.close()


def test_progressive_id_matte_follows_the_frames_own_counts():
    import torch
    region = (8, 8, 48, 40)   # 5 x 4 tiles over the objects
    c = fresh(blob_of(OBJECTS))
    try:
        with c.progressive(region, 8) as prog:
            prog.advance(2)
            mask = np.zeros(prog.tile_shape, bool)
            mask[::2, 1::2] = True
            prog.advance_tiles(5, mask)
            mask2 = np.zeros(prog.tile_shape, bool)
            mask2[1, :] = True
            prog.advance_tiles(8, mask2)
            ns = prog.read()[2]
            assert sorted(np.unique(ns).tolist()) == [2, 5, 8], np.unique(ns)
            for key in KEYS:
                dev = prog.idmatte_device(key)
                c.synchronize()
                dev = host(dev)
                want = c.idmatte_device(region, 8, key, ns=torch.from_numpy(ns.view(np.int32)).cuda())
                c.synchronize()
                assert not same_planes(dev, host(want)), key
                assert np.array_equal(dev["samples"].view(np.uint32), ns)
                assert int(occupied(dev).max()) >= 2
    finally:
        c.close()


def test_more_nodes_than_slots_overflow_into_other():
    """tests/golden/idmatte/grid.xml: 144 spheres, each a node, under 4x4 pixels: a pixel's 64 samples meet nine nodes"""
    region, spp = (0, 0, 4, 4), 64
    c = fresh(blob_of(GRID, None))
    try:
        hit, ids2 = route(c, region, spp)
        distinct = np.array([[len(set(ids2[y, x, :, 0][hit[y, x]].tolist())) for x in range(4)] for y in range(4)])
        print("distinct nodes per pixel:\n", distinct)
        assert (distinct > SLOTS).all()
        for key in KEYS:
            got = c.idmatte(region, spp, key)
            assert not same_planes(got, route_planes(hit, ids2, key)), key
        node = c.idmatte(region, spp, "node")
        print("other:\n", node["other"])
        assert (node["other"] > 0).any() and (occupied(node) == SLOTS).all()
        assert np.array_equal(node["counts"].sum(axis=-1) + node["other"], hit.sum(axis=-1))
        assert int(occupied(c.idmatte(region, spp, "material")).max()) == 2   # two materials, row by row
    finally:
        c.close()


def test_select_is_the_restatement_and_the_full_list_is_the_coverage(cases):
    import torch
    from qaray_amd import hip
    from qaray_amd.host import HostScene, SCENES_DIR
    region, spp, _ = CASES[OBJECTS]
    c = fresh(blob_of(OBJECTS))
    try:
        dev = c.idmatte_device(region, spp, "node")
        c.synchronize()
        m = host(dev)
        assert not same_planes(m, cases[OBJECTS]["node"])
        present = sorted(set(m["ids"].ravel().tolist()) - {EMPTY})
        assert len(present) >= 3
        grey = torch.zeros(m["samples"].shape, dtype=torch.uint8, device="cuda:0")
        for name, sel in {"empty": [], "absent": [500, -7], "one": present[:1], "two and absent": present[:2] + [999], "full": present}.items():
            got = c.idmatte_select_device(dev["ids"], dev["counts"], dev["samples"], sel, out_bytes=grey)
            c.synchronize()
            got = got.cpu().numpy()
            want = select_ref(m["ids"], m["counts"], m["samples"], sel)
            assert got.dtype == F32 and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), name
            assert np.array_equal(got, hip.idmatte_select_host(m["ids"], m["counts"], m["samples"], sel)), name
            assert np.array_equal(grey.cpu().numpy(), linear_byte(want)), name
            if name == "full":
                whole = m["other"] == 0
                assert whole.sum() > whole.size // 2 and np.array_equal(got.view(np.uint32)[whole], cases[OBJECTS]["coverage"].view(np.uint32)[whole])
            if name == "one":
                assert ((got > 0) & (got < 1)).any()   # an anti-aliased edge
        # the node pick() names has positive coverage at its pixel; the name-to-index lookup names the same node
        hs = HostScene(os.path.join(SCENES_DIR, OBJECTS), size=SIZE)
        try:
            teapot = hs.node_index("teapot-high.obj")
        finally:
            hs.close()
        picked = set()
        for (px, py) in ((region[0] + 3, region[1] + 2), (region[0] + 12, region[1] + 8), (region[0] + 20, region[1] + 13)):
            node = hip.pick(c, px, py)[0]
            if node < 0:
                continue
            picked.add(node)
            cov = c.idmatte_select_device(dev["ids"], dev["counts"], dev["samples"], [node])
            c.synchronize()
            assert float(cov[py - region[1], px - region[0]]) > 0, (px, py, node)
        assert picked and picked <= set(present), (picked, present)
        assert 0 < teapot < len(hip.blob_table(blob_of(OBJECTS), "instances"))
    finally:
        c.close()


def test_refusals_write_nothing():
    import torch
    from qaray_amd import hip
    L = hip.lib()
    region = (5, 3, 45, 27)
    h, w = region[3] - region[1], region[2] - region[0]

    def sentinels():
        return {k: torch.full((h, w, SLOTS) if k in ("ids", "counts") else (h, w), 7, dtype=torch.int32, device="cuda:0") for k in hip.IDMATTE_PLANES}

    c = fresh(blob_of(BOX))
    try:
        t = sentinels()
        ptr = [t[k].data_ptr() for k in hip.IDMATTE_PLANES]
        assert L.qa_idmatte_region_device(c._h, *region, 4, None, 0, None, None, None, None, None) == QA_EINVAL      # no plane
        assert L.qa_idmatte_region_device(c._h, *region, 0, None, 0, *ptr, None) == QA_EINVAL                       # spp = 0
        assert L.qa_idmatte_region_device(c._h, *region, 4, None, 2, *ptr, None) == QA_EINVAL                       # no such key
        assert L.qa_idmatte_region_device(c._h, *region, 4, None, 0, ptr[0] + 4, *ptr[1:], None) == QA_EINVAL       # ids not 16-byte aligned
        for bad in ((5, 3, 5, 27), (-1, 0, 10, 10), (0, 0, SIZE[0] + 1, 10)):
            assert L.qa_idmatte_region_device(c._h, *bad, 4, None, 0, *ptr, None) == QA_EINVAL, bad
        assert L.qa_idmatte_select_device(c._h, ptr[0], ptr[1], ptr[3], h * w, None, 1, ptr[2], None, None) == QA_EINVAL   # a list of one id, null
        assert L.qa_idmatte_select_device(c._h, ptr[0], ptr[1], ptr[3], h * w, None, 0, None, None, None) == QA_EINVAL     # no output
        with pytest.raises(ValueError):
            c.idmatte(region, 4, key="colour")
        c.synchronize()
        torch.cuda.synchronize()
        assert all(bool((v == 7).all()) for v in t.values())
        one = c.idmatte_device(region, 4, other=t["other"])   # a single plane is the full call's
        c.synchronize()
        assert list(one) == ["other"] and bool((t["ids"] == 7).all())
    finally:
        c.close()
    # a camera with depth of field
    d = fresh(blob_of(DOF_SCENE))
    try:
        assert float(hip.blob_camera(blob_of(DOF_SCENE))["dof"]) > 0.1
        t = sentinels()
        with pytest.raises(hip.HipError) as e:
            d.idmatte_device(region, 4, **t)
        assert e.value.code == QA_EUNSUPPORTED
        with pytest.raises(hip.HipError) as e:
            d.idmatte(region, 4)
        assert e.value.code == QA_EUNSUPPORTED
        with d.progressive(region, 2) as prog:
            prog.advance(1)
            with pytest.raises(hip.HipError) as e:
                prog.idmatte_device(**t)
            assert e.value.code == QA_EUNSUPPORTED
        d.synchronize()
        torch.cuda.synchronize()
        assert all(bool((v == 7).all()) for v in t.values())
    finally:
        d.close()


def test_cli_matte_node_writes_the_nodes_coverage_and_leaves_the_three(tmp_path):
    from PIL import Image
    from qaray_amd.host import SCENES_DIR, HostScene
    import torch
    exe = os.path.join(ROOT, "qaray_amd", "lib", "qaray_hip")
    size = (48, 36)
    common = ["-batch", "-spp", "4", "-bounce", "5", "-size", str(size[0]), str(size[1]), "-root", SCENES_DIR]
    names = ("colorBuffer.png", "depthBuffer.png", "sampleBuffer.png")
    run = lambda args: subprocess.run([exe] + common + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)   # noqa: E731
    outs = {}
    for mode, extra in (("plain", []), ("matte", ["-matte-node", "lightPlane"]), ("prog", ["-matte-node", "lightPlane", "-progressive", "2"])):
        outs[mode] = str(tmp_path / mode) + "_"
        r = run(extra + ["-out", outs[mode], os.path.join(SCENES_DIR, BOX)])
        assert r.returncode == 0, r.stdout
    assert not os.path.exists(outs["plain"] + "matte_lightPlane.png")
    for mode in ("matte", "prog"):
        for png in names:
            with open(outs["plain"] + png, "rb") as a, open(outs[mode] + png, "rb") as b:
                assert a.read() == b.read(), (mode, png)
    img = Image.open(outs["matte"] + "matte_lightPlane.png")
    assert img.mode == "L" and img.size == size
    grey = np.asarray(img)
    hs = HostScene(os.path.join(SCENES_DIR, BOX), size=size)
    try:
        light = hs.node_index("lightPlane")
        blob = hs.flatten()
    finally:
        hs.close()
    c = fresh(blob)
    try:
        m = c.idmatte_device((0, 0) + size, 4, "node")
        cov = c.idmatte_select_device(m["ids"], m["counts"], m["samples"], [light])
        c.synchronize()
        cov = cov.cpu().numpy()
    finally:
        c.close()
    assert np.array_equal(grey, linear_byte(cov))
    print("grey levels of the light's matte:", np.unique(grey).tolist())
    assert (grey > 0).any() and (grey == 0).any()   # the light, and the rest
    with open(outs["matte"] + "matte_lightPlane.png", "rb") as a, open(outs["prog"] + "matte_lightPlane.png", "rb") as b:
        assert a.read() == b.read()
    r = run(["-matte-node", "lightPlane", "-devices", "1", os.path.join(SCENES_DIR, BOX)])
    assert r.returncode != 0 and "-matte-node" in r.stdout and "-devices" in r.stdout
    r = run(["-matte-node", "noSuchNode", "-out", str(tmp_path / "none") + "_", os.path.join(SCENES_DIR, BOX)])
    assert r.returncode != 0 and "noSuchNode" in r.stdout and not os.path.exists(str(tmp_path / "none") + "_colorBuffer.png")
    assert torch.cuda.is_available()
