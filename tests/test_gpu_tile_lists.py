"""Camera rays of LDS-resident scenes on per-tile leaf lists (option "tile_lists", qaray_amd/csrc/hip/qa_tilecull.h and
qa_kernel.h): every frame here is rendered with the lists off, with them on, and by the counting kernel (the reference's tree,
walked as the reference walks it), and the three must agree bit for bit - colour, first-hit depth and sample counts as 32-bit
words, and the samples / casts_normal / casts_shadow counters.  Where the path cannot run (depth of field, a mesh without an
own tree or with more than 64 leaves, a scene that is not resident, the lit and textured variants) it must step aside and
leave the same frames."""
import os

import numpy as np
import pytest

import scene_fuzz_util as fz
from conftest import bits, golden_blob, load_golden
from tile_list_util import POSES, pose_blob

pytestmark = pytest.mark.gpu

COUNTERS = ("samples", "casts_normal", "casts_shadow")
BOX = "example_project12_box.xml"


@pytest.fixture(scope="module")
def ctx():
    from qaray_amd import hip
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def default_options(ctx):
    yield
    for name, v in (("tile_lists", -1), ("chunk_spp", -1), ("chunk_tail", 0)):
        ctx.set_option(name, v)


def words(frame, cnt):
    rgb, depth, ns = frame
    return bits(rgb), bits(depth), np.ascontiguousarray(ns).view(np.uint32), tuple(cnt[k] for k in COUNTERS)


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def three_ways(ctx, blob, region, spp, spp_max=None, bounce=5, on=-1, render=None):
    """Uploads `blob` and renders `region` with the lists off, on (limit `on`) and by the counting kernel -> the frame, checked
    to be the same three times.  render(ctx, stats) -> (rgb, depth, ns) replaces the plain region render."""
    ctx.upload_scene(blob)
    render = render or (lambda c, stats: c.render_region(region, spp, max_bounce=bounce, spp_max=spp_max, stats=stats))
    got = {}
    for mode, (limit, stats) in {"off": (0, False), "on": (on, False), "counting": (on, True)}.items():
        ctx.set_option("tile_lists", limit)
        ctx.reset_counters()
        frame = render(ctx, stats)
        got[mode] = words(frame, ctx.counters())
        assert ("counting" in ctx.kernel_name()) == stats, ctx.kernel_name()
    assert same(got["on"], got["off"]), "tile lists on differ from off"
    assert same(got["on"], got["counting"]), "tile lists on differ from the counting kernel"
    return got["on"]


def box_blob(size):
    from qaray_amd.host import load_scene_blob
    return load_scene_blob(BOX, size=size)


def scene_from_text(tmp_path, text, size, files=()):
    """A scene file written from `text` (assets: scenes/, or `files` = {name: text} beside it) -> blob."""
    from qaray_amd.host import SCENES_DIR, load_scene_blob
    p = tmp_path / "scene.xml"
    p.write_text(text)
    for name, body in dict(files).items():
        (tmp_path / name).write_text(body)
    return load_scene_blob(str(p), size=size, asset_root=str(tmp_path) if files else SCENES_DIR)


def box_xml(objects, camera=None):
    """The Cornell box's file with `objects` in place of its mesh node (the emissive plane and the camera stay)."""
    from qaray_amd.host import SCENES_DIR
    text = open(os.path.join(SCENES_DIR, BOX)).read()
    a, b = text.index("<object type=\"obj\""), text.index("<object type=\"plane\"")
    return text[:a] + objects + "\n    " + text[b:]


BOX_NODE = """<object type="obj" name="%s">
      <translate x="-278" y="-274.4" z="-279.1"/>
      <scale value="%s"/>
      <rotate angle="90" x="1"/>
      <rotate angle="180" z="1"/>
      <translate x="%s" y="%s" z="11"/>
    </object>"""


def test_box_equals_its_golden(ctx):
    rgb, depth, ns, meta = load_golden("c2_box_64x64_4spp")
    assert ctx is not None
    got = three_ways(ctx, golden_blob(meta), tuple(meta["crop"]), meta["spp_min"], spp_max=meta["spp_max"], bounce=meta["bounce"])
    assert ctx.kernel_name().startswith("qa_integrate<RES=1,LIGHTS=0"), ctx.kernel_name()
    assert np.array_equal(got[0], bits(rgb)) and np.array_equal(got[1], bits(depth)) and np.array_equal(got[2], ns.view(np.uint32))
    assert got[3] == (meta["samples"], meta["casts_normal"], meta["casts_shadow"])


def test_ragged_region_at_an_odd_offset(ctx):
    """61x45 pixels from (13, 7): ragged tiles on the right and at the bottom, and no tile starts on a multiple of 8."""
    blob = box_blob((152, 150))
    got = three_ways(ctx, blob, (13, 7, 74, 52), 4)
    whole = ctx.render_region((0, 0, 152, 150), 4)
    assert np.array_equal(got[0], bits(whole[0][7:52, 13:74])) and np.array_equal(got[1], bits(whole[1][7:52, 13:74]))


def test_strips_of_rank_1_of_3(ctx):
    import torch
    from qaray_amd import hip
    w, h, spp = 152, 150, 4

    def strips(c, stats):
        rows = hip.strip_count(0, h, 1, 3) * 8
        rgb = torch.zeros((rows, w, 3), dtype=torch.float32, device="cuda")
        depth = torch.zeros((rows, w), dtype=torch.float32, device="cuda")
        ns = torch.zeros((rows, w), dtype=torch.int32, device="cuda")
        c.render_strips_device((0, 0, w, h), 1, 3, spp, rgb, depth, ns, stats=stats)
        c.synchronize()
        return rgb.cpu().numpy(), depth.cpu().numpy(), ns.cpu().numpy()

    got = three_ways(ctx, box_blob((w, h)), None, spp, render=strips)
    whole = ctx.render_region((0, 0, w, h), spp)
    for k, y in enumerate(range(8, h, 24)):      # strips 1, 4, 7, ...
        n = min(8, h - y)
        assert np.array_equal(got[0].reshape(-1, w, 3)[k * 8:k * 8 + n], bits(whole[0][y:y + n]))


def test_every_hand_over_rebuilds_the_lists(ctx):
    """chunk_spp = 1 on a frame of 64 tiles - fewer than waves: a tile changes hands after every sample, and whoever takes
    it builds its lists again."""
    ctx.set_option("chunk_spp", 1)
    ctx.set_option("chunk_tail", 1)
    got = three_ways(ctx, box_blob((64, 64)), (0, 0, 64, 64), 4)
    ctx.set_option("chunk_spp", 0)
    assert same(got, three_ways(ctx, box_blob((64, 64)), (0, 0, 64, 64), 4))


def test_adaptive_sampling(ctx):
    rgb, depth, ns, meta = load_golden("sphere_adaptive_64x48_4to32spp")      # no mesh: nothing to list
    got = three_ways(ctx, golden_blob(meta), tuple(meta["crop"]), meta["spp_min"], spp_max=meta["spp_max"], bounce=meta["bounce"])
    assert np.array_equal(got[2], ns.view(np.uint32)) and np.array_equal(got[1], bits(depth))
    got = three_ways(ctx, box_blob((64, 48)), (0, 0, 64, 48), 4, spp_max=24)   # the box: lanes of a tile end at different samples
    assert got[2].min() < got[2].max()


@pytest.mark.parametrize("limit", [1, 2, 24])
def test_list_tiles_and_walk_tiles_in_one_frame(ctx, limit):
    """With a limit of one leaf most tiles of the box walk the tree and some use their list; 24 = every tile that fits the area."""
    got = three_ways(ctx, box_blob((152, 150)), (0, 0, 152, 150), 4, on=limit)
    ctx.set_option("tile_lists", -1)
    ctx.reset_counters()
    assert same(got, words(ctx.render_region((0, 0, 152, 150), 4), ctx.counters()))


@pytest.mark.parametrize("pose", POSES)
def test_five_poses(ctx, pose):
    three_ways(ctx, pose_blob(pose, (48, 36)), (0, 0, 48, 36), 4)


def test_two_mesh_instances(ctx, tmp_path):
    """Two nodes show the same mesh, one behind and beside the other: two lists per tile, one area."""
    objects = BOX_NODE % ("examples/cornell_box.obj", "0.05", "0", "0") + "\n    " + BOX_NODE % ("examples/cornell_box.obj", "0.03", "9", "30")
    blob = scene_from_text(tmp_path, box_xml(objects), (96, 72))
    three_ways(ctx, blob, (0, 0, 96, 72), 4)
    assert ctx.kernel_name().startswith("qa_integrate<RES=1,LIGHTS=0"), ctx.kernel_name()
    three_ways(ctx, blob, (0, 0, 96, 72), 2, on=24)


def test_plane_in_front_of_the_mesh(ctx, tmp_path):
    """A plane node before the mesh in the scene graph covers part of it: those camera rays reach the mesh holding a finite distance."""
    plane = """<object type="plane" name="screen">
      <rotate angle="90" x="1"/>
      <scale value="6"/>
      <translate x="-5" y="-20" z="8"/>
    </object>
    """
    blob = scene_from_text(tmp_path, box_xml(plane + BOX_NODE % ("examples/cornell_box.obj", "0.05", "0", "0")), (96, 72))
    got = three_ways(ctx, blob, (0, 0, 96, 72), 4)
    alone = three_ways(ctx, box_blob((96, 72)), (0, 0, 96, 72), 4)
    assert not np.array_equal(got[1], alone[1])      # the plane is in the picture


def scatter_obj(n):
    """n separate triangles over the Cornell box's floor area: the own tree gives every one a leaf."""
    v, f = [], []
    for t in range(n):
        i, j = t % 9, t // 9
        x, y, z = 30 + 55.0 * i, 20.0 * ((i * 7 + j * 3) % 5), 30 + 60.0 * j
        v += ["v %g %g %g" % (x, y, z), "v %g %g %g" % (x + 30, y, z), "v %g %g %g" % (x, y + 10, z + 30)]
        f += ["f %d %d %d" % (3 * t + 1, 3 * t + 3, 3 * t + 2)]
    return "\n".join(v + f) + "\n"


NEEDLE_OBJ = """v 0 0 0
v 556 0 0
v 556 0 559
v 0 0 559
v 100 300 100
v 400 300 100
v 250 300.0005 100
f 1 3 2
f 1 4 3
f 5 6 7
"""


def test_steps_aside(ctx, tmp_path):
    # depth of field: the camera rays of a tile share no origin
    rgb, depth, ns, meta = load_golden("softshadow_dof_60x45_2spp")
    three_ways(ctx, golden_blob(meta), tuple(meta["crop"]), meta["spp_min"], spp_max=meta["spp_max"], bounce=meta["bounce"])
    # a mesh with a needle of a triangle keeps the reference tree (useFast = 0): no leaf table
    (tmp_path / "a").mkdir()
    blob = scene_from_text(tmp_path / "a", box_xml(BOX_NODE % ("needle.obj", "0.05", "0", "0")), (64, 48), files={"needle.obj": NEEDLE_OBJ})
    three_ways(ctx, blob, (0, 0, 64, 48), 4)
    assert ctx.kernel_name().startswith("qa_integrate<RES=1,LIGHTS=0"), ctx.kernel_name()
    # a resident mesh of 70 triangles in 70 leaves, more than the 64 a leaf table holds: none either
    (tmp_path / "b").mkdir()
    blob = scene_from_text(tmp_path / "b", box_xml(BOX_NODE % ("scatter.obj", "0.05", "0", "0")), (64, 48), files={"scatter.obj": scatter_obj(70)})
    three_ways(ctx, blob, (0, 0, 64, 48), 4)
    assert ctx.kernel_name().startswith("qa_integrate<RES=1,LIGHTS=0"), ctx.kernel_name()
    # a scene in global memory
    rgb, depth, ns, meta = load_golden("c3_object_1080p_crop_2spp")
    three_ways(ctx, golden_blob(meta), tuple(meta["crop"]), meta["spp_min"], spp_max=meta["spp_max"], bounce=meta["bounce"])
    assert "RES=0" in ctx.kernel_name() or "qa_integrate_cs" in ctx.kernel_name(), ctx.kernel_name()


# resident scenes with mesh nodes among the generated ones (tests/scene_fuzz_util.py); theirs are the lit and textured kernel
# variants, which carry no list code: the option must leave them what the manifest records
FUZZ = [("transforms", 0), ("transforms", 1), ("lights", 0), ("camera", 0), ("camera", 3), ("contact", 0)]


@pytest.mark.parametrize("case", FUZZ, ids=fz.case_id)
def test_fuzz_scenes_equal_their_records(ctx, case):
    e, o = fz.manifest()[case], fz.oracle_frame(*case)
    p = o["params"]
    got = three_ways(ctx, o["blob"], (0, 0, p["width"], p["height"]), p["spp_min"], spp_max=p["spp_max"], bounce=p["bounce"], on=24)
    assert "RES=1" in ctx.kernel_name(), ctx.kernel_name()
    assert fz.sha(got[1].tobytes()) == e["depth_sha256"] and fz.sha(got[2].tobytes()) == e["ns_sha256"]
    assert got[3] == (e["samples"], e["casts_normal"], e["casts_shadow"])
