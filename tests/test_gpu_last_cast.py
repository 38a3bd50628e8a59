"""The last cast of a path in a resident scene without lights, asked as "which emitter does this ray meet" (option "last_cast",
qaray_amd/csrc/hip/qa_kernel.h lastCastQuery): every frame here is rendered with the option off (the same kernel runs the
closest-hit sweep and shading), with it on, and by the counting kernel (the reference's tree, walked as the reference walks it),
and the three must agree bit for bit - colour, first-hit depth and sample counts as 32-bit words, and the samples / casts_normal /
casts_shadow counters.  kernel_name() names the variant exactly where the scene predicate holds."""
import numpy as np
import pytest

from cast_cost_util import BOX_NODE, MIXED, SCREEN, scene_blob as cast_cost_blob
from conftest import bits
from last_cast_util import SCENES, SPOILED, mesh_materials, scene_blob, spoil
from tile_list_util import POSES, pose_blob

pytestmark = pytest.mark.gpu

COUNTERS = ("samples", "casts_normal", "casts_shadow")
FRAMES = ((152, 150), (61, 45))   # whole tiles and a row of half ones | ragged tiles on both sides
VARIANT = "qa_integrate<RES=1,LIGHTS=0,TEX=0,AREA=0,LASTCAST=1>"
PLAIN = "qa_integrate<RES=1,LIGHTS=0,TEX=0,AREA=0>"
OPTIONS = (("last_cast", -1), ("tile_lists", -1), ("chunk_spp", -1), ("chunk_tail", 0))


@pytest.fixture(scope="module")
def ctx():
    from qaray_amd import hip
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def default_options(ctx):
    yield
    for name, v in OPTIONS:
        ctx.set_option(name, v)


def words(frame, cnt):
    rgb, depth, ns = frame
    return bits(rgb), bits(depth), np.ascontiguousarray(ns).view(np.uint32), tuple(cnt[k] for k in COUNTERS)


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def three_ways(ctx, region, spp, bounce=5, spp_max=None, name=VARIANT):
    """The uploaded scene's `region` with the query off, on and by the counting kernel -> the frame, the same three times."""
    got = {}
    for mode, (on, stats) in {"off": (0, False), "on": (1, False), "counting": (1, True)}.items():
        ctx.set_option("last_cast", on)
        ctx.reset_counters()
        got[mode] = words(ctx.render_region(region, spp, max_bounce=bounce, spp_max=spp_max, stats=stats), ctx.counters())
        assert ctx.kernel_name() == (PLAIN + " counting variant (STATS=1, reference tree)" if stats else name), ctx.kernel_name()
    assert same(got["on"], got["off"]), "the query's frame differs from the closest-hit sweep's"
    assert same(got["on"], got["counting"]), "the query's frame differs from the counting kernel's"
    return got["on"]


def all_bounces(ctx, blob, size, label, name=VARIANT):
    ctx.upload_scene(blob)
    assert ctx.kernel_name() == name, (label, ctx.kernel_name())
    frames = {b: three_ways(ctx, (0, 0) + size, 4, bounce=b, name=name) for b in (5, 1, 0)}
    assert same(frames[5], frames[1]), label   # a path of such a scene is a camera ray and one bounce ray
    assert frames[0][3][1] == frames[0][3][0], label   # no bounce: one cast per sample
    return frames


@pytest.mark.parametrize("size", FRAMES, ids=lambda s: "%dx%d" % s)
def test_poses_and_cast_cost_scenes(ctx, tmp_path, size):
    blobs = {pose: pose_blob(pose, size) for pose in POSES}
    blobs["mixed"] = cast_cost_blob(tmp_path, MIXED, size)
    blobs["mixed_inside"] = cast_cost_blob(tmp_path, MIXED, size, "inside")
    blobs["mixed_beside"] = cast_cost_blob(tmp_path, MIXED, size, "beside")
    blobs["screen"] = cast_cost_blob(tmp_path, SCREEN + BOX_NODE, size)
    blobs["light_quad"] = cast_cost_blob(tmp_path, BOX_NODE, size, "under_the_light")
    bounced = 0
    for name, blob in blobs.items():
        # (the screen is a plane without a material: a hit on it ends the path without a draw, and the scene keeps the plain variant)
        f = all_bounces(ctx, blob, size, name, PLAIN if name == "screen" else VARIANT)
        bounced += f[5][3][1] > f[5][3][0]
    assert bounced >= 7, bounced   # (beside the box the camera sees its outer wall: those bounce rays are few or none)


@pytest.mark.parametrize("size", FRAMES, ids=lambda s: "%dx%d" % s)
def test_scenes_made_to_trip_the_query(ctx, tmp_path, size):
    for name in sorted(SCENES):
        f = all_bounces(ctx, scene_blob(tmp_path, name, size), size, name)
        assert f[5][3][1] > f[5][3][0], name
        assert np.isfinite(f[5][0].view(np.float32)).all(), name
    # the environment's colour reaches the picture through the rays that leave the box
    a = all_bounces(ctx, scene_blob(tmp_path, "open_environment", size), size, "open")[5]
    b = all_bounces(ctx, scene_blob(tmp_path, "glow_before_mesh", size), size, "closed")[5]
    assert not np.array_equal(a[0], b[0])


def test_variant_runs_exactly_where_the_predicate_holds(ctx):
    size = (61, 45)
    ctx.upload_scene(pose_blob("box", size))
    assert ctx.kernel_name() == VARIANT
    for how in SPOILED:
        ctx.upload_scene(spoil(pose_blob("box", size), how))
        assert ctx.kernel_name() == PLAIN, (how, ctx.kernel_name())
        three_ways(ctx, (0, 0) + size, 4, name=PLAIN)   # the option changes nothing there
    from qaray_amd.host import load_scene_blob
    ctx.upload_scene(load_scene_blob("example_project3_box.xml", size=size))   # the box with lights
    assert "LASTCAST" not in ctx.kernel_name() and "LIGHTS=1" in ctx.kernel_name(), ctx.kernel_name()


def test_one_sample_chunks(ctx):
    ctx.upload_scene(pose_blob("box", (152, 150)))
    whole = three_ways(ctx, (0, 0, 152, 150), 4)
    ctx.set_option("chunk_spp", 1)
    ctx.set_option("chunk_tail", 1)
    assert same(three_ways(ctx, (0, 0, 152, 150), 4), whole)


def test_adaptive_sampling(ctx):
    ctx.upload_scene(pose_blob("box", (64, 48)))
    got = three_ways(ctx, (0, 0, 64, 48), 4, spp_max=24)
    assert got[2].min() < got[2].max()   # the lanes of a tile end at different samples


def test_tile_lists_off(ctx):
    ctx.upload_scene(pose_blob("box", (152, 150)))
    with_lists = three_ways(ctx, (0, 0, 152, 150), 4)
    ctx.set_option("tile_lists", 0)
    assert same(three_ways(ctx, (0, 0, 152, 150), 4), with_lists)


def test_material_edit_leaves_the_variant_and_returns(ctx):
    """A wall made reflective on the resident scene: the plan loses lastCastQuery and the frames come from the plain variant;
    edited back, the variant returns with the frame it gave before."""
    from qaray_amd import hip
    size = (61, 45)
    blob = pose_blob("box", size)
    ctx.upload_scene(blob)
    before = three_ways(ctx, (0, 0) + size, 4)
    wall = mesh_materials(blob)[1]
    plain = hip.blob_table(blob, "materials")[wall:wall + 1].copy()
    shiny = plain.copy()
    shiny["reflection"]["color"] = 0.375
    ctx.edit_materials(wall, shiny)
    assert ctx.kernel_name() == PLAIN, ctx.kernel_name()
    edited = three_ways(ctx, (0, 0) + size, 4, name=PLAIN)
    assert not same(edited, before)
    ctx.edit_materials(wall, plain)
    assert ctx.kernel_name() == VARIANT, ctx.kernel_name()
    assert same(three_ways(ctx, (0, 0) + size, 4), before)
