"""qa_integrate_lastcast runs one sample per turn of its loop (qaray_amd/csrc/hip/qa_kernel_lastcast_body.h: camera ray, closest
hit, shading, the bounce ray's query, sample end - no per-lane state machine).  The places where that text differs from the general
body's: which lanes hold a pixel, option sync_samples, the lens draws ahead of the camera ray, lanes of a tile that end at different
samples while every sample is a hand-over, bounce rays that take the second trip, and sums that start from 0 with a -0 term.  Every
frame is rendered three ways as in test_gpu_last_cast.py - query off, query on, counting kernel - and the three must agree bit for
bit: colour, first-hit depth and sample counts as 32-bit words, and the samples / casts_normal / casts_shadow counters."""
import os

import numpy as np
import pytest

from last_cast_util import scene_blob
from test_gpu_last_cast import VARIANT, same, three_ways
from tile_list_util import BOX, pose_blob

pytestmark = pytest.mark.gpu

OPTIONS = (("last_cast", -1), ("tile_lists", -1), ("chunk_spp", -1), ("chunk_tail", 0), ("sync_samples", -1))
SPP = 4


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


def upload(ctx, blob):
    ctx.upload_scene(blob)
    assert ctx.kernel_name() == VARIANT, ctx.kernel_name()


@pytest.mark.parametrize("size", ((1, 1), (9, 1), (8, 9)), ids=lambda s: "%dx%d" % s)
def test_smallest_frames(ctx, size):
    """One lane holds a pixel; a second tile of one pixel next to a row of eight (63 and 55 padding lanes); a second tile row of one
    pixel row."""
    upload(ctx, pose_blob("box", size))
    got = three_ways(ctx, (0, 0) + size, SPP)
    assert got[3][0] == size[0] * size[1] * SPP
    assert (got[2] == SPP).all()


def test_sync_samples_changes_nothing(ctx):
    size = (61, 45)
    upload(ctx, pose_blob("box", size))
    frames = []
    for v in (0, 1):
        ctx.set_option("sync_samples", v)
        frames.append(three_ways(ctx, (0, 0) + size, SPP))
    assert same(frames[0], frames[1])
    assert frames[0][3][1] > frames[0][3][0]   # bounce rays were cast


def test_depth_of_field(ctx):
    """The lens draws come ahead of the camera ray from the pixel's stream; tile lists are off for such a camera."""
    from qaray_amd import hip
    from qaray_amd.host import HostScene, SCENES_DIR
    size = (61, 45)
    blob = pose_blob("box", size)
    hs = HostScene(os.path.join(SCENES_DIR, BOX), size=size)
    try:
        hs.set_camera((0, -65, 11), (0, 0, 11), up=(0, 0, 1), focaldist=60.0, dof=0.6)
        hip.blob_camera(blob)[...] = hs.camera()
    finally:
        hs.close()
    assert float(hip.blob_camera(blob)["dof"]) > 0.1
    upload(ctx, blob)
    lens = three_ways(ctx, (0, 0) + size, SPP)
    upload(ctx, pose_blob("box", size))
    assert not same(three_ways(ctx, (0, 0) + size, SPP), lens)


def test_adaptive_sampling_in_one_sample_chunks(ctx):
    """Lanes of a tile end at different samples, and every sample is a hand-over."""
    size = (64, 48)
    upload(ctx, pose_blob("box", size))
    whole = three_ways(ctx, (0, 0) + size, SPP, spp_max=24)
    assert whole[2].min() < whole[2].max()
    ctx.set_option("chunk_spp", 1)
    ctx.set_option("chunk_tail", 1)
    assert same(three_ways(ctx, (0, 0) + size, SPP, spp_max=24), whole)


def test_rays_that_ask_again(ctx, tmp_path):
    """coplanar_after: the glow plane lies in the plane of the mesh's light quad, and the host model finds bounce rays whose query
    says "ask again" there (profiles/leaf_sweep_cost.txt 1) - they take the second trip.  The frames of option off and on agree,
    and so does casts_normal (three_ways)."""
    size = (152, 150)
    upload(ctx, scene_blob(tmp_path, "coplanar_after", size))
    got = three_ways(ctx, (0, 0) + size, SPP)
    assert got[3][1] > got[3][0]
    assert np.isfinite(got[0].view(np.float32)).all()


def test_minus_zero_terms(ctx):
    """L = 0 + T * c with c = -0 is +0, not c: the emission of the emitting plane, the background and the environment each have a
    -0.0 component."""
    from qaray_amd import hip
    size = (61, 45)
    blob = pose_blob("box", size)
    inst, sets, mats = hip.blob_table(blob, "instances"), hip.blob_table(blob, "mtlsets"), hip.blob_table(blob, "materials")
    planes = [k for k in range(1, len(inst)) if inst[k]["obj_type"] == 2]
    glow = [int(sets[inst[k]["mtlset"]]["first"]) for k in planes if mats[sets[inst[k]["mtlset"]]["first"]]["emission"]["color"].any()]
    assert glow, "the box has an emitting plane"
    mats[glow[0]]["emission"]["color"] = (15.0, -0.0, 7.0)
    background, environment = hip.blob_backdrop(blob)
    background["color"] = (-0.0, 0.25, 0.5)
    environment["color"] = (0.5, 0.25, -0.0)
    assert np.signbit(hip.blob_backdrop(blob)[0]["color"][0]) and np.signbit(mats[glow[0]]["emission"]["color"][1])
    upload(ctx, blob)
    got = three_ways(ctx, (0, 0) + size, SPP)
    assert got[3][1] > got[3][0]
