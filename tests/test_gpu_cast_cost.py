"""A cast on an LDS-resident mesh with its two shortcuts (qaray_amd/csrc/hip/qa_kernel.h: the own tree's slab step in fma form,
and the leaf test that trusts the found triangle at entry <= t) against the counting kernel, which walks the reference's tree as
the reference does: colour, first-hit depth and sample counts as 32-bit words and the samples / casts_normal / casts_shadow
counters, bit for bit, with the tile lists off and at their default limit.  The first-hit planes and the ray queries compile the
same walk: they must meet what the counting kernel's first cast meets."""
import numpy as np
import pytest

from conftest import bits
from cast_cost_util import BOX_NODE, MIXED, SCREEN, scene_blob
from test_gpu_tile_lists import box_blob, same, three_ways, words
from tile_list_util import POSES, pose_blob

pytestmark = pytest.mark.gpu

FRAMES = ((152, 150), (61, 45))   # whole tiles and a row of half ones | ragged tiles on both sides


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


def blobs(tmp_path, size):
    """name -> blob at `size`: the five poses, the mixed scene from outside, from inside the room and from beside the box, the box
    behind a plane, the view up at the mesh's light quad"""
    out = {pose: pose_blob(pose, size) for pose in POSES}
    out["mixed"] = scene_blob(tmp_path, MIXED, size)
    out["mixed_inside"] = scene_blob(tmp_path, MIXED, size, "inside")
    out["mixed_beside"] = scene_blob(tmp_path, MIXED, size, "beside")
    out["screen"] = scene_blob(tmp_path, SCREEN + BOX_NODE, size)
    out["light_quad"] = scene_blob(tmp_path, BOX_NODE, size, "under_the_light")
    return out


@pytest.mark.parametrize("size", FRAMES, ids=lambda s: "%dx%d" % s)
def test_frames_equal_the_counting_kernel(ctx, tmp_path, size):
    w, h = size
    for name, blob in blobs(tmp_path, size).items():
        on = three_ways(ctx, blob, (0, 0, w, h), 4, on=8)   # lists off, limit 8, counting
        assert ctx.kernel_name().startswith("qa_integrate<RES=1,LIGHTS=0"), (name, ctx.kernel_name())
        if name == "light_quad":   # the mesh's light quad fills the view: most camera casts of the mesh end on element 15
            assert on[3][0] > 0 and np.isfinite(on[1].view(np.float32)).all()
        if name == "mixed":
            ids = ctx.gbuffer((0, 0, w, h))["ids"][..., 0]
            assert len(np.unique(ids[ids >= 0])) >= 3, np.unique(ids)   # sphere, plane and mesh are all in the picture


def test_one_sample_chunks(ctx):
    ctx.set_option("chunk_spp", 1)
    ctx.set_option("chunk_tail", 1)
    got = three_ways(ctx, box_blob((152, 150)), (0, 0, 152, 150), 4, on=8)
    ctx.set_option("chunk_spp", -1)
    ctx.set_option("chunk_tail", 0)
    ctx.set_option("tile_lists", -1)
    ctx.reset_counters()
    assert same(got, words(ctx.render_region((0, 0, 152, 150), 4), ctx.counters()))


def test_first_hit_planes_and_ray_queries_share_the_walk(ctx, tmp_path):
    """One sample, no bounce: the counting kernel's depth plane is the reference's first hit.  The guide planes' depth is that
    plane, and the camera rays of sample 0, cast as a batch, end at that distance on that node."""
    w, h = 152, 150
    region = (0, 0, w, h)
    for name, blob in blobs(tmp_path, (w, h)).items():
        ctx.upload_scene(blob)
        depth = ctx.render_region(region, 1, max_bounce=0, stats=True)[1]
        assert "counting" in ctx.kernel_name(), ctx.kernel_name()
        g = ctx.gbuffer(region)
        assert np.array_equal(bits(g["depth"]), bits(depth)), name
        o, d = ctx.camera_rays(region)
        r = ctx.cast_rays(o, d)
        hit = (g["ids"][..., 0] >= 0).reshape(-1)
        assert hit.sum() > w * h // 8, (name, int(hit.sum()))
        assert np.array_equal(r["ids"][:, 0], g["ids"][..., 0].reshape(-1)), name
        assert np.array_equal(bits(r["t"])[hit], bits(depth).reshape(-1)[hit]), name
