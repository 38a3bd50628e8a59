"""The leaf sweep of the last-cast query (option "leaf_sweep", qaray_amd/csrc/hip/qa_kernel.h sweepLeaves: a bounce ray of
qa_integrate_lastcast tests every box of a small mesh's leaf table once and then the triangles of its own candidates, instead of
walking the mesh's own tree): every frame here is rendered with the option off (the walk), with it on, and by the counting kernel
(the reference's tree, walked as the reference walks it), and the three must agree bit for bit - colour, first-hit depth and
sample counts as 32-bit words, and the samples / casts_normal / casts_shadow counters."""
import numpy as np
import pytest

from cast_cost_util import BOX_NODE, MIXED, scene_blob as cast_cost_blob
from last_cast_util import SCENES, scene_blob
from leaf_sweep_util import scene_blob as table_blob
from test_gpu_last_cast import FRAMES, PLAIN, VARIANT, same, words
from tile_list_util import POSES, pose_blob

pytestmark = pytest.mark.gpu

OPTIONS = (("leaf_sweep", -1), ("last_cast", -1), ("tile_lists", -1), ("chunk_spp", -1), ("chunk_tail", 0))


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


def three_ways(ctx, region, spp, bounce=5, spp_max=None, last_cast=1):
    """The uploaded scene's `region` with the sweep off, on and by the counting kernel -> the frame, the same three times."""
    got = {}
    for mode, (on, stats) in {"off": (0, False), "on": (1, False), "counting": (1, True)}.items():
        ctx.set_option("last_cast", last_cast)
        ctx.set_option("leaf_sweep", on)
        ctx.reset_counters()
        got[mode] = words(ctx.render_region(region, spp, max_bounce=bounce, spp_max=spp_max, stats=stats), ctx.counters())
        assert ctx.kernel_name() == (PLAIN + " counting variant (STATS=1, reference tree)" if stats else VARIANT), ctx.kernel_name()
    assert same(got["on"], got["off"]), "the sweep's frame differs from the walk's"
    assert same(got["on"], got["counting"]), "the sweep's frame differs from the counting kernel's"
    return got["on"]


def all_bounces(ctx, blob, size, label):
    ctx.upload_scene(blob)
    assert ctx.kernel_name() == VARIANT, (label, ctx.kernel_name())
    frames = {b: three_ways(ctx, (0, 0) + size, 4, bounce=b) for b in (5, 1, 0)}
    assert same(frames[5], frames[1]), label   # a path of such a scene is a camera ray and one bounce ray
    assert frames[0][3][1] == frames[0][3][0], label   # no bounce: one cast per sample
    return frames


@pytest.mark.parametrize("size", FRAMES, ids=lambda s: "%dx%d" % s)
def test_poses_and_cast_cost_scenes(ctx, tmp_path, size):
    blobs = {pose: pose_blob(pose, size) for pose in POSES}
    blobs["mixed"] = cast_cost_blob(tmp_path, MIXED, size)
    blobs["mixed_inside"] = cast_cost_blob(tmp_path, MIXED, size, "inside")
    blobs["mixed_beside"] = cast_cost_blob(tmp_path, MIXED, size, "beside")
    blobs["light_quad"] = cast_cost_blob(tmp_path, BOX_NODE, size, "under_the_light")
    bounced = 0
    for name, blob in blobs.items():
        f = all_bounces(ctx, blob, size, name)
        bounced += f[5][3][1] > f[5][3][0]
    # (as in test_gpu_last_cast.py, which asks 7 of these and the screen scene: up to three - the cameras beside the box, which see
    # its outer wall, and partly behind it - may have few bounce rays or none)
    assert bounced >= 6, bounced


@pytest.mark.parametrize("size", FRAMES, ids=lambda s: "%dx%d" % s)
def test_scenes_made_to_trip_the_query(ctx, tmp_path, size):
    for name in sorted(SCENES):
        f = all_bounces(ctx, scene_blob(tmp_path, name, size), size, name)
        assert f[5][3][1] > f[5][3][0], name
        assert np.isfinite(f[5][0].view(np.float32)).all(), name


def test_adaptive_sampling(ctx):
    ctx.upload_scene(pose_blob("box", (64, 48)))
    got = three_ways(ctx, (0, 0, 64, 48), 2, spp_max=6)
    assert got[2].min() < got[2].max()   # the lanes of a tile end at different samples


def test_one_sample_chunks(ctx):
    """A pixel's state is handed on between waves with the sweep on."""
    ctx.upload_scene(pose_blob("box", (152, 150)))
    whole = three_ways(ctx, (0, 0, 152, 150), 4)
    ctx.set_option("chunk_spp", 1)
    ctx.set_option("chunk_tail", 1)
    assert same(three_ways(ctx, (0, 0, 152, 150), 4), whole)


def test_inert_where_its_carrier_is_off(ctx):
    """tile_lists 0: the camera rays walk the tree, the bounce rays still sweep.  last_cast 0: no ray is asked the query, and the
    option changes nothing."""
    ctx.upload_scene(pose_blob("box", (152, 150)))
    usual = three_ways(ctx, (0, 0, 152, 150), 4)
    ctx.set_option("tile_lists", 0)
    assert same(three_ways(ctx, (0, 0, 152, 150), 4), usual)
    ctx.set_option("tile_lists", -1)
    assert same(three_ways(ctx, (0, 0, 152, 150), 4, last_cast=0), usual)


@pytest.mark.parametrize("name", ("one_leaf", "many_leaves"))
def test_meshes_without_a_table_to_sweep(ctx, tmp_path, name):
    """An own tree that is one leaf, and one of more leaves than a leaf table holds: the same bits through the walk."""
    for size in FRAMES:
        f = all_bounces(ctx, table_blob(tmp_path, name, size), size, name)
        assert f[5][3][1] > f[5][3][0], name


def test_option_values(ctx):
    """-1 (auto), 0 and 1 are taken; the kernel's name does not say which."""
    size = (61, 45)
    ctx.upload_scene(pose_blob("box", size))
    frames = []
    for v in (-1, 0, 1, 7, -3):
        ctx.set_option("leaf_sweep", v)
        ctx.reset_counters()
        frames.append(words(ctx.render_region((0, 0) + size, 4), ctx.counters()))
        assert ctx.kernel_name() == VARIANT
    assert all(same(f, frames[0]) for f in frames)
