"""The first-hit guide planes (qa_gbuffer_region*, qa_progressive_gbuffer_device: qa_gbuffer.hip) against the renderer, the oracle
and float64 geometry.  Frames of 64x48, the odd region (5, 3) - (52, 43).  Which scene reaches which <RES, TEX> instantiation of
qa_gbuffer is listed in gbuffer_util.SCENES and asserted here against kernel_name() (the G-buffer launcher uses the frame
launcher's predicate: plan.resident, plan.textured)."""
import numpy as np
import pytest

from gbuffer_util import MISS, REGION, SCENES, SEEDS, SIZE, bits, emission_twin, scene_blob

pytestmark = pytest.mark.gpu
QA_EINVAL = -1
QA_ENOSCENE = -5
BOX = "example_project12_box.xml"
SPHERES = "example_project3_sphere.xml"


def fresh(blob):
    from qaray_amd import hip
    c = hip.Context(0)
    c.set_option("coop", 0)   # (kernel_name() then names qa_integrate<RES=..,TEX=..> for every scene)
    c.upload_scene(blob)
    return c


@pytest.fixture(scope="module")
def planes():
    """scene -> (blob, {seed: G-buffer of REGION}, kernel name)"""
    out = {}
    for scene in SCENES:
        blob = scene_blob(scene)
        c = fresh(blob)
        try:
            out[scene] = (blob, {seed: c.gbuffer(REGION, seed) for seed in SEEDS}, c.kernel_name())
        finally:
            c.close()
    return out


def test_every_instantiation_is_reached(planes):
    seen = set()
    for scene, want in SCENES.items():
        name = planes[scene][2]
        got = (int("RES=1" in name), int("TEX=1" in name))
        seen.add(got)
        assert want is None or got == want, (scene, name)
    assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)}, seen


@pytest.mark.parametrize("scene", list(SCENES))
def test_depth_is_the_renderers_and_the_oracles(planes, scene):
    from oracle import binding as oracle
    blob, g, _ = planes[scene]
    c = fresh(blob)
    try:
        for seed in SEEDS:
            depth = c.render_region(REGION, 1, max_bounce=0, seed=seed)[1]
            assert np.array_equal(bits(g[seed]["depth"]), bits(depth)), (scene, seed)
            assert np.array_equal(bits(g[seed]["depth"]), bits(oracle.render(blob, REGION, 1, max_bounce=0, seed=seed)[1])), (scene, seed)
    finally:
        c.close()


def test_depth_with_a_dof_camera_follows_the_rng_draws():
    from oracle import binding as oracle
    from qaray_amd import hip
    from qaray_amd.host import HostScene, SCENES_DIR
    import os
    blob = scene_blob(BOX)
    hs = HostScene(os.path.join(SCENES_DIR, BOX), size=SIZE)
    hs.set_camera((0, -65, 11), (0, 0, 11), up=(0, 0, 1), focaldist=60.0, dof=0.6)   # the scene's own view, with a lens
    cam = hs.camera()
    assert float(cam["dof"]) > 0.1
    c = fresh(blob)
    try:
        c.edit_camera(cam)
        edited = c.download_scene()
        for seed in SEEDS:
            g = c.gbuffer(REGION, seed)
            assert np.array_equal(bits(g["depth"]), bits(c.render_region(REGION, 1, max_bounce=0, seed=seed)[1]))
            assert np.array_equal(bits(g["depth"]), bits(oracle.render(edited, REGION, 1, max_bounce=0, seed=seed)[1]))
        assert not np.array_equal(c.gbuffer(REGION, SEEDS[0])["depth"], c.gbuffer(REGION, SEEDS[1])["depth"])   # the draws show
    finally:
        c.close()


@pytest.mark.parametrize("scene", list(SCENES))
def test_albedo_is_the_oracles_twin_frame_on_hits_and_its_backdrop_on_misses(planes, scene):
    from oracle import binding as oracle
    blob, g, _ = planes[scene]
    seed = SEEDS[0]
    twin = oracle.render(emission_twin(blob), REGION, 1, max_bounce=0, seed=seed)[0].astype(np.float32)
    orig = oracle.render(blob, REGION, 1, max_bounce=0, seed=seed)[0].astype(np.float32)
    hit = g[seed]["depth"] != MISS
    a = g[seed]["albedo"]
    print(scene, "hit pixels", hit.sum(), "miss", (~hit).sum())
    assert np.array_equal(bits(a)[hit], bits(twin)[hit])
    assert np.array_equal(bits(a)[~hit], bits(orig)[~hit])


def camera_rays(blob, region):
    """float64 camera rays of sample 0 (no depth of field): origin, unit directions [h, w, 3]"""
    from oracle import binding as oracle
    from qaray_amd import hip
    cam = hip.blob_camera(blob)
    x0, y0, x1, y1 = region
    ys, xs = np.mgrid[y0:y1, x0:x1].astype(np.float64)
    hx, hy = float(np.float32(oracle.halton(0, 11))), float(np.float32(oracle.halton(0, 13)))
    A, U, V = (cam[k].astype(np.float64) for k in ("screenA", "screenU", "screenV"))
    pt = A + U * (xs + hx)[..., None] + V * (ys + hy)[..., None]
    o = cam["cam_pos"].astype(np.float64)
    d = pt - o
    return o, d / np.linalg.norm(d, axis=2, keepdims=True)


def analytic_normals(blob, g, region):
    """float64 world normals of the sphere and plane hits, from the blob's instance transforms, the camera ray and the depth plane;
    -> (normals, mask of the pixels covered)"""
    from qaray_amd import hip
    inst = hip.blob_table(blob, "instances")
    o, d = camera_rays(blob, region)
    p = o + d * g["depth"].astype(np.float64)[..., None]
    out = np.zeros_like(p)
    done = np.zeros(p.shape[:2], bool)
    for k in np.unique(g["ids"][..., 0]):
        if k < 0 or inst[k]["obj_type"] not in (1, 2):
            continue
        chain = []
        a = int(k)
        while a >= 0:
            chain.append(a)
            a = int(inst[a]["parent"])
        m = g["ids"][..., 0] == k
        q = p[m]
        for a in reversed(chain):   # root first: into the node's space
            itm = inst[a]["itm"].astype(np.float64).reshape(3, 3).T
            q = (q - inst[a]["pos"].astype(np.float64)) @ itm.T
        n = q / np.linalg.norm(q, axis=1, keepdims=True) if inst[k]["obj_type"] == 1 else np.tile([0.0, 0.0, 1.0], (len(q), 1))
        for a in chain:             # node first: back out, normals through the inverse transpose
            itm = inst[a]["itm"].astype(np.float64).reshape(3, 3).T
            n = n @ itm
            n /= np.linalg.norm(n, axis=1, keepdims=True)
        out[m] = n
        done |= m
    return out, done


# 16 x the largest deviation measured on the device (9.15e-5 rad, one run on an MI355X: 1 325 pixels of example_project3_sphere.xml,
# the worst on the floor sphere scaled (70, 70, 0.5), where the fp32 depth moves the float64 hit point along a thin ellipsoid)
# would be 1.5e-3; the bound is never looser than 1e-4 rad, so that is what is asserted.  The margin is thin on that one sphere: a change of the compiler's rounding there can cross it, and then the thing to look at
# is that sphere's depth, not the normal's transform
NORMAL_ANGLE_BOUND = 1e-4


def test_normals_of_spheres_and_planes_match_float64_geometry():
    """Angle between the kernel's normal and the float64 one: the bound is 1e-4 rad (an untransformed, unnormalised or flipped
    normal misses by orders of magnitude); the largest deviation is printed."""
    blob = scene_blob(SPHERES)
    c = fresh(blob)
    try:
        g = c.gbuffer(REGION, SEEDS[0])
    finally:
        c.close()
    want, done = analytic_normals(blob, g, REGION)
    hit = g["depth"] != MISS
    assert done.sum() > 300 and not (done & ~hit).any()
    n = g["normal"].astype(np.float64)
    assert np.abs(1 - np.linalg.norm(n[hit], axis=1)).max() < 1e-6
    assert not bits(g["normal"])[~hit].any()   # exactly +0
    cosang = np.clip((n[done] * want[done]).sum(axis=1), -1, 1)
    ang = np.arccos(cosang)
    cross = np.linalg.norm(np.cross(n[done], want[done]), axis=1)   # (accurate for small angles)
    print("largest normal deviation [rad]:", cross.max(), "pixels", done.sum())
    assert cosang.min() > 0 and cross.max() < NORMAL_ANGLE_BOUND, (ang.max(), cross.max())


def obj_polygons(path):
    """-> the polygons of a Wavefront file, float64 [k, 3] each (v and f lines; negative indices count back from the last vertex)"""
    v, polys = [], []
    for line in open(path):
        t = line.split("#")[0].split()
        if t and t[0] == "v":
            v.append([float(x) for x in t[1:4]])
        elif t and t[0] == "f":
            idx = [int(x.split("/")[0]) for x in t[1:]]
            polys.append(np.float64([v[i - 1] if i > 0 else v[len(v) + i] for i in idx]))
    return polys


def face_normals(blob, g, region, node, polys):
    """float64 world normals of the faces the pixels of mesh node `node` see: the polygons through the node's instance transforms,
    the hit point from the camera ray and the depth plane, the polygon that contains it.  A quad of the file that is not planar
    (the Cornell box's walls: 549.6 / 552.8 / 556.0) is shaded with normals interpolated between its corners', so its normal here is
    the mean of its four corner normals and its tolerance the largest angle between a corner's and the mean.
    -> (normals, mask of the pixels covered: on one face and at least 0.5 away from every other face's plane, tolerance [rad])"""
    from qaray_amd import hip
    inst = hip.blob_table(blob, "instances")
    o, d = camera_rays(blob, region)
    pt = o + d * g["depth"].astype(np.float64)[..., None]
    m = g["ids"][..., 0] == node
    q = pt[m]
    best, second = np.full(len(q), np.inf), np.full(len(q), np.inf)
    out, tol = np.zeros((len(q), 3)), np.zeros(len(q))
    for p in polys:
        a = node
        while a >= 0:   # node first, then its parents: into world space
            p = p @ inst[a]["tm"].astype(np.float64).reshape(3, 3) + inst[a]["pos"].astype(np.float64)
            a = int(inst[a]["parent"])
        corner = np.float64([np.cross(p[k] - p[k - 1], p[(k + 1) % len(p)] - p[k]) for k in range(len(p))])
        corner /= np.linalg.norm(corner, axis=1, keepdims=True)
        n = corner.sum(axis=0)
        n /= np.linalg.norm(n)
        dist = np.abs((q - p[0]) @ n)
        for k in range(len(p)):
            e = p[(k + 1) % len(p)] - p[k]
            dist = np.where(np.cross(e, q - p[k]) @ n >= -1e-3 * np.linalg.norm(e), dist, np.inf)
        take = dist < best
        second = np.where(take, best, np.minimum(second, dist))
        out[take], tol[take] = n, np.linalg.norm(np.cross(corner, n), axis=1).max()
        best = np.where(take, dist, best)
    full, done, ftol = np.zeros(pt.shape), np.zeros(m.shape, bool), np.zeros(m.shape)
    full[m], done[m], ftol[m] = out, (best < 0.15) & (second > 0.5), tol
    return full, done, ftol


def test_box_normals_are_the_mesh_faces_normals(planes):
    """The RES mesh path against float64 face normals from cornell_box.obj through the blob's instance transforms.  On the planar
    faces the bound is NORMAL_ANGLE_BOUND (largest deviation 7.6e-8 rad on 3 077 pixels of a 64x64 frame, one run on an MI355X); on
    the three quads of the file that are not planar the interpolated normal may turn by the quad's own bend (4.1e-3 rad) on top of
    it.  A flipped, untransformed or wrongly interpolated normal misses by orders of magnitude.  Pixels within 0.5 of a second
    face's plane (corners and edges) are left out; at least 85 % of the mesh's pixels must remain."""
    import os
    from qaray_amd.host import SCENES_DIR
    blob, gs, _ = planes[BOX]
    g = gs[SEEDS[0]]
    node = 1
    want, done, tol = face_normals(blob, g, REGION, node, obj_polygons(os.path.join(SCENES_DIR, "examples", "cornell_box.obj")))
    seen = g["ids"][..., 0] == node
    assert seen.sum() > 1000 and done.sum() > 0.85 * seen.sum(), (seen.sum(), done.sum())
    n = g["normal"].astype(np.float64)
    cross = np.linalg.norm(np.cross(n[done], want[done]), axis=1)
    planar = tol[done] < 1e-9
    print("largest normal deviation [rad] on planar faces:", cross[planar].max(), "pixels", planar.sum(), "; on bent quads:", cross[~planar].max() if (~planar).any() else None,
          "pixels", (~planar).sum(), "bend", tol[done].max())
    assert planar.sum() > 0.5 * done.sum()
    assert ((n[done] * want[done]).sum(axis=1) > 0).all()
    assert (cross <= tol[done] + NORMAL_ANGLE_BOUND).all(), (cross - tol[done]).max()


def test_box_normals_are_unit_and_zero_on_misses(planes):
    g = planes[BOX][1][SEEDS[0]]
    hit = g["depth"] != MISS
    assert np.abs(1 - np.linalg.norm(g["normal"][hit].astype(np.float64), axis=1)).max() < 1e-6
    assert not bits(g["normal"])[~hit].any()


@pytest.mark.parametrize("scene", list(SCENES))
def test_ids_name_the_node_and_its_material(planes, scene):
    from qaray_amd import hip
    blob, g, _ = planes[scene]
    ids, hit = g[SEEDS[0]]["ids"], g[SEEDS[0]]["depth"] != MISS
    inst, sets = hip.blob_table(blob, "instances"), hip.blob_table(blob, "mtlsets")
    assert (ids[~hit] == -1).all()
    node, word = ids[hit][:, 0], ids[hit][:, 1]
    assert (node > 0).all() and (node < len(inst)).all() and (inst[node]["obj_type"] != 0).all()
    mat = np.where(word < 0, word, word & ~hip.QA_GBUFFER_BACKFACE)
    ms = inst[node]["mtlset"]
    none = ms < 0
    assert (mat[none] == -1).all()
    s = sets[np.maximum(ms, 0)]
    single = ~none & (s["multi"] == 0)
    assert np.array_equal(mat[single], s["first"][single])
    multi = ~none & (s["multi"] != 0)   # first + mtlID, or the white case
    assert (((mat[multi] >= s["first"][multi]) & (mat[multi] < s["first"][multi] + s["count"][multi])) | (mat[multi] == -2)).all()
    print(scene, "single", single.sum(), "multi", multi.sum(), "none", none.sum(), "white", (mat == -2).sum())
    if scene == BOX:   # the Cornell box is a multi-material mesh: first + mtlID is exercised, and with more than one mtlID
        assert multi.sum() > 1000 and len(np.unique(mat[multi])) >= 3
    # the id is tied to the albedo plane: where the material's diffuse has no texture, its colour IS the albedo - a wrong mtlID
    # offset names a material of another colour (the box's walls are white, red and green)
    mats = hip.blob_table(blob, "materials")
    plain = (mat >= 0) & (mats[np.maximum(mat, 0)]["diffuse"]["texmap"] < 0)
    albedo = g[SEEDS[0]]["albedo"][hit]
    assert np.array_equal(bits(albedo[plain]), bits(mats[mat[plain]]["diffuse"]["color"]))
    assert (bits(albedo[mat == -1]) == 0).all() and (albedo[mat == -2] == 1).all()
    if scene == BOX:
        assert plain.sum() == (mat >= 0).sum() > 500


def test_back_face_bit_inside_a_sphere():
    """The camera moved to the centre of the scene's first sphere: every pixel that sees that sphere sees its inside."""
    from qaray_amd import hip
    from qaray_amd.host import HostScene, SCENES_DIR
    import os
    blob = scene_blob(SPHERES)
    inst = hip.blob_table(blob, "instances")
    k = int(np.flatnonzero(inst["obj_type"] == 1)[0])
    centre = np.zeros(3)
    a = k
    while a >= 0:
        centre = centre @ inst[a]["tm"].astype(np.float64).reshape(3, 3) + inst[a]["pos"]
        a = int(inst[a]["parent"])
    hs = HostScene(os.path.join(SCENES_DIR, SPHERES), size=SIZE)
    hs.set_camera(centre, centre + np.array([0.0, 1.0, 0.0]), up=(0, 0, 1))
    c = fresh(blob)
    try:
        front = c.gbuffer(REGION, SEEDS[0])["ids"]
        c.edit_camera(hs.camera())
        ids = c.gbuffer(REGION, SEEDS[0])["ids"]
    finally:
        c.close()
    assert (ids[..., 0] == k).all()
    assert (ids[..., 1] >= hip.QA_GBUFFER_BACKFACE).all()
    seen = front[front[..., 0] == k]
    assert len(seen) and (seen[:, 1] < hip.QA_GBUFFER_BACKFACE).all() and (seen[:, 1] >= 0).all()


def test_after_an_edit_the_planes_are_those_of_the_edited_blob():
    import torch
    from qaray_amd import hip
    blob = scene_blob(BOX)
    c = fresh(blob)
    try:
        with c.progressive(REGION, 2, seed=SEEDS[1]) as prog:
            prog.advance(1)
            inst = hip.blob_table(blob, "instances").copy()
            k = int(np.flatnonzero(inst["obj_type"] != 0)[-1])
            inst[k]["pos"] += np.float32([0.5, 0.0, 0.25])
            c.edit_instances(k, inst[k:k + 1])
            mats = hip.blob_table(blob, "materials").copy()
            mats[0]["diffuse"]["color"] = np.float32([0.1, 0.7, 0.3])
            c.edit_materials(0, mats[0:1])
            edited = c.download_scene()
            got = c.gbuffer(REGION, SEEDS[1])
            prog.restart()
            dev = prog.gbuffer_device()
            c.synchronize()
            torch.cuda.synchronize()
            dev = {k_: v.cpu().numpy() for k_, v in dev.items()}
        c2 = fresh(edited)
        try:
            want = c2.gbuffer(REGION, SEEDS[1])
            before = fresh(blob)
            try:
                old = before.gbuffer(REGION, SEEDS[1])
            finally:
                before.close()
        finally:
            c2.close()
    finally:
        c.close()
    for name in hip.GBUFFER_PLANES:
        assert np.array_equal(bits(got[name]), bits(want[name])), name
        assert np.array_equal(bits(dev[name]), bits(want[name])), name
    assert not np.array_equal(old["depth"], want["depth"]) and not np.array_equal(old["albedo"], want["albedo"])


def test_single_planes_errors_counters_and_frames_untouched(planes):
    import torch
    from qaray_amd import hip
    blob, g, _ = planes[BOX]
    c = fresh(blob)
    try:
        frame0 = c.render_region(REGION, 2, seed=SEEDS[0])
        cnt0 = c.counters()
        for name in hip.GBUFFER_PLANES:
            one = c.gbuffer_device(REGION, SEEDS[0], **{name: torch.empty(g[SEEDS[0]][name].shape, dtype=torch.int32 if name == "ids" else torch.float32,
                                                                        device="cuda:0")})
            c.synchronize()
            assert list(one) == [name] and np.array_equal(bits(one[name].cpu().numpy()), bits(g[SEEDS[0]][name])), name
        assert c.counters() == cnt0
        frame1 = c.render_region(REGION, 2, seed=SEEDS[0])
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(frame0, frame1))
        L = hip.lib()
        d = torch.empty(47 * 40, dtype=torch.float32, device="cuda:0")
        assert L.qa_gbuffer_region_device(c._h, 5, 3, 52, 43, 1, None, None, None, None, None) == QA_EINVAL
        for bad in ((5, 3, 5, 43), (5, 3, 52, 3), (-1, 0, 10, 10), (0, 0, SIZE[0] + 1, 10), (0, 0, 10, SIZE[1] + 1)):
            assert L.qa_gbuffer_region_device(c._h, *bad, 1, None, None, d.data_ptr(), None, None) == QA_EINVAL, bad
            with pytest.raises(hip.HipError) as e:
                c.gbuffer(bad, 1)
            assert e.value.code == QA_EINVAL
        host = np.zeros(64, np.float32)
        assert L.qa_gbuffer_region(c._h, -1, 0, 1 << 30, 1 << 30, 1, None, None, host.ctypes.data, None) == QA_EINVAL   # (nothing is sized by it)
        empty = hip.Context(0)
        try:
            assert L.qa_gbuffer_region_device(empty._h, 0, 0, 8, 8, 1, None, None, d.data_ptr(), None, None) == QA_ENOSCENE
            host = np.zeros(64, np.float32)
            assert L.qa_gbuffer_region(empty._h, 0, 0, 8, 8, 1, None, None, host.ctypes.data, None) == QA_ENOSCENE
        finally:
            empty.close()
    finally:
        c.close()


def test_pick_agrees_with_the_planes(planes):
    from qaray_amd import hip
    blob, gs, _ = planes[BOX]
    g = gs[SEEDS[0]]
    c = fresh(blob)
    try:
        hit = np.argwhere(g["depth"] != MISS)
        miss = np.argwhere(g["depth"] == MISS)
        assert len(hit) and len(miss), "the scene must show both a hit and a miss in the region"
        for (y, x) in (tuple(hit[len(hit) // 2]), tuple(miss[0]), (0, 0), (39, 46)):
            node, mat, depth = hip.pick(c, REGION[0] + int(x), REGION[1] + int(y), SEEDS[0])
            assert (node, mat) == tuple(int(v) for v in g["ids"][y, x]) and np.float32(depth) == g["depth"][y, x]
    finally:
        c.close()
