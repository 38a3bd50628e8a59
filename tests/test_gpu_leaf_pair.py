"""The leaf sweep of the last-cast query with a leaf per turn (qaray_amd/csrc/hip/qa_kernel.h sweepLeaves: a lane reads
where its candidate leaf's triangles are from one byte in LDS and tests both of them in straight-line code): every frame here is
rendered with option "leaf_sweep" off (the walk), with it on, and by the counting kernel (the reference's tree, walked as the
reference walks it), and the three must agree bit for bit - colour, first-hit depth and sample counts as 32-bit words, and the
samples / casts_normal / casts_shadow counters - as in tests/test_gpu_leaf_sweep.py, whose comparison this is."""
import pytest

from last_cast_util import scene_blob
from leaf_pair_util import odd_floor_blob
from leaf_sweep_util import scene_blob as table_blob
from test_gpu_last_cast import VARIANT, same
from test_gpu_leaf_sweep import OPTIONS, three_ways
from tile_list_util import pose_blob

pytestmark = pytest.mark.gpu

SIZE = (152, 150)


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


def bounced(frame):
    return frame[3][1] > frame[3][0]   # more casts than samples: bounce rays were asked


def test_the_box(ctx):
    ctx.upload_scene(pose_blob("box", SIZE))
    assert ctx.kernel_name() == VARIANT
    assert bounced(three_ways(ctx, (0, 0) + SIZE, 4))


@pytest.mark.parametrize("name", ("coplanar_after", "coplanar_before"))
def test_the_coplanar_scenes(ctx, tmp_path, name):
    """The glow plane lies in the plane of the mesh's light quad: triangles at exactly the query's limit, ties."""
    ctx.upload_scene(scene_blob(tmp_path, name, SIZE))
    assert ctx.kernel_name() == VARIANT
    assert bounced(three_ways(ctx, (0, 0) + SIZE, 4))


def test_a_leaf_of_one_triangle_in_the_second_of_two_swept_meshes(ctx, tmp_path):
    """The box and a floor of five triangles: both meshes are swept (the second one's bytes lie behind the first's), and the
    floor's own tree has a leaf of one triangle and a leaf that ends at the mesh's last record."""
    ctx.upload_scene(odd_floor_blob(tmp_path, SIZE))
    assert ctx.kernel_name() == VARIANT
    assert bounced(three_ways(ctx, (0, 0) + SIZE, 4))


def test_a_swept_mesh_beside_a_walked_one(ctx, tmp_path):
    """The box (swept) and a floor whose own tree is one leaf (walked)."""
    ctx.upload_scene(table_blob(tmp_path, "one_leaf", SIZE))
    assert ctx.kernel_name() == VARIANT
    assert bounced(three_ways(ctx, (0, 0) + SIZE, 4))


def test_a_ragged_frame_in_one_sample_chunks(ctx):
    """150x147: ragged tiles on both sides; a pixel's state is handed on between waves after every sample."""
    size = (150, 147)
    ctx.upload_scene(pose_blob("box", size))
    whole = three_ways(ctx, (0, 0) + size, 4)
    ctx.set_option("chunk_spp", 1)
    ctx.set_option("chunk_tail", 1)
    assert same(three_ways(ctx, (0, 0) + size, 4), whole)
