"""One-shot frames of qa_integrate_lastcast finish the 8x8 tiles no camera ray can hit anything from in closed form (option
"empty_tiles", qaray_amd/csrc/hip/qa_emptytile.h and qa_kernel_lastcast_body.h section A): rgb = background, depth = QA_BIGFLOAT,
ns = spp_min, their samples and casts counted as the frame holds them.  Every frame here is wide, so that there are such tiles
(the box at the reference's 608x600 has none), and is rendered with the option on and off and by the CPU oracle: colour, first-hit
depth and sample counts agree as 32-bit words, and so do the samples / casts_normal / pixels counters.  The decision itself is read
from qa_empty_tiles_device, which runs the kernel's device function once per tile."""
import numpy as np
import pytest

from conftest import bits
from empty_tile_util import background_of, scene_blob, tile_all

pytestmark = pytest.mark.gpu

COUNTERS = ("samples", "casts_normal", "pixels")
WIDE, SMALL = (192, 64), (128, 48)
VARIANT = "qa_integrate<RES=1,LIGHTS=0,TEX=0,AREA=0,LASTCAST=1>"
OPTIONS = (("empty_tiles", -1), ("tile_lists", -1), ("chunk_spp", -1), ("chunk_tail", 0))


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


@pytest.fixture(scope="module")
def blobs(tmp_path_factory):
    d = tmp_path_factory.mktemp("empty_tiles")
    made = {}

    def get(name, size):
        if (name, size) not in made:
            made[name, size] = scene_blob(d, name, size)
        return made[name, size]
    return get


_oracle = {}


def oracle_words(blob, name, size, region, spp, spp_max=None):
    """The oracle's frame of `region`, computed once per (scene, size, region, sampling) and shared."""
    from oracle import binding as oracle
    key = (name, size, region, spp, spp_max)
    if key not in _oracle:
        rgb, depth, ns, cnt = oracle.render(blob, region, spp, spp_max=spp_max)
        pixels = (region[2] - region[0]) * (region[3] - region[1])   # (the oracle finishes every pixel of the region and keeps no count)
        _oracle[key] = (bits(rgb), bits(depth), np.ascontiguousarray(ns).view(np.uint32), (int(cnt.samples), int(cnt.casts_normal), pixels))
    return _oracle[key]


def words(frame, cnt):
    rgb, depth, ns = frame
    return bits(rgb), bits(depth), np.ascontiguousarray(ns).view(np.uint32), tuple(int(cnt[k]) for k in COUNTERS)


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def on_and_off(ctx, render):
    """render(ctx) -> (rgb, depth, ns) with the option on and off -> the frame, checked to be the same twice."""
    got = {}
    for mode, v in (("on", 1), ("off", 0)):
        ctx.set_option("empty_tiles", v)
        ctx.reset_counters()
        got[mode] = words(render(ctx), ctx.counters())
        assert ctx.kernel_name() == VARIANT, ctx.kernel_name()
    ctx.set_option("empty_tiles", -1)
    assert same(got["on"], got["off"]), "empty tiles in closed form differ from the traced ones"
    return got["on"]


def three_ways(ctx, blobs, name, size, region, spp, spp_max=None):
    blob = blobs(name, size)
    ctx.upload_scene(blob)
    got = on_and_off(ctx, lambda c: c.render_region(region, spp, spp_max=spp_max))
    assert same(got, oracle_words(blob, name, size, region, spp, spp_max)), "the frame differs from the oracle's"
    return got


def background_tiles(blob, w, spp, size):
    """bool [ty, tx]: every pixel of the tile is the background's bits, QA_BIGFLOAT deep and has spp samples in the frame `w`."""
    pure = (w[0] == bits(background_of(blob))).all(axis=2) & (w[1] == bits(np.float32(1.0e30))) & (w[2] == spp)
    return tile_all(pure, size)


def test_three_way_frame(ctx, blobs):
    region = (0, 0) + WIDE
    got = three_ways(ctx, blobs, "box", WIDE, region, 16)
    mask = ctx.empty_tiles(region)
    assert mask.shape == (8, 24) and mask.any() and not mask.all()
    pure = background_tiles(blobs("box", WIDE), oracle_words(blobs("box", WIDE), "box", WIDE, region, 16), 16, WIDE)
    assert not (mask & ~pure).any()
    from qaray_amd import hip
    assert np.array_equal(mask, hip.empty_tiles_host(blobs("box", WIDE), region))   # the host build of the header decides alike
    # derived, not traced, and still what the frame holds: every pixel has its 16 samples
    assert got[3][0] == 16 * WIDE[0] * WIDE[1] and got[3][2] == WIDE[0] * WIDE[1]
    ctx.set_option("empty_tiles", 0)
    assert not ctx.empty_tiles(region).any()
    ctx.set_option("empty_tiles", -1)
    ctx.set_option("tile_lists", 0)   # the test's pyramid lives in the lists' LDS row: no lists, no empty tile
    assert not ctx.empty_tiles(region).any()


def test_off_grid_region(ctx, blobs):
    """Ragged tiles on the left, right, top and bottom: no tile starts on a multiple of 8, the last column is 6 wide, the last row 2 high."""
    region = (5, 3, 187, 61)
    got = three_ways(ctx, blobs, "box", WIDE, region, 16)
    mask = ctx.empty_tiles(region)
    assert mask.shape == (8, 23) and mask[:, -1].all() and mask[-1].any() and not mask.all()
    whole = oracle_words(blobs("box", WIDE), "box", WIDE, (0, 0) + WIDE, 16)
    assert np.array_equal(got[0], whole[0][3:61, 5:187]) and np.array_equal(got[2], whole[2][3:61, 5:187])


def test_strips_of_rank_1_of_3(ctx, blobs):
    import torch
    from qaray_amd import hip
    w, h = WIDE
    ctx.upload_scene(blobs("box", WIDE))

    def strips(c):
        rows = hip.strip_count(0, h, 1, 3) * 8
        rgb = torch.zeros((rows, w, 3), dtype=torch.float32, device="cuda")
        depth = torch.zeros((rows, w), dtype=torch.float32, device="cuda")
        ns = torch.zeros((rows, w), dtype=torch.int32, device="cuda")
        c.render_strips_device((0, 0, w, h), 1, 3, 16, rgb, depth, ns)
        c.synchronize()
        return rgb.cpu().numpy(), depth.cpu().numpy(), ns.cpu().numpy()

    got = on_and_off(ctx, strips)
    whole = oracle_words(blobs("box", WIDE), "box", WIDE, (0, 0) + WIDE, 16)
    rows = np.concatenate([np.arange(y, y + 8) for y in range(8, h, 24)])   # strips 1, 4, 7
    for k in range(3):
        assert np.array_equal(got[k], whole[k][rows])
    assert np.array_equal(ctx.empty_tiles((0, 0, w, h), 1, 3), ctx.empty_tiles((0, 0, w, h))[1::3])


@pytest.mark.timeout(120)
def test_forced_chunking(ctx, blobs):
    """chunk_spp 4, chunk_tail 4 at 16 spp: every tile has four work items, and the three later ones of an empty tile must neither
    wait for a publish that never comes nor touch the pixels (a wait that ran into its bound would take minutes: the timeout)."""
    region = (0, 0) + WIDE
    whole = three_ways(ctx, blobs, "box", WIDE, region, 16)
    ctx.set_option("chunk_spp", 4)
    ctx.set_option("chunk_tail", 4)
    assert same(three_ways(ctx, blobs, "box", WIDE, region, 16), whole)


def test_adaptive_sampling(ctx, blobs):
    region = (0, 0) + WIDE
    got = three_ways(ctx, blobs, "box", WIDE, region, 4, spp_max=16)
    mask = ctx.empty_tiles(region)
    ns = got[2].reshape(8, 8, 24, 8).transpose(0, 2, 1, 3)
    assert (ns[mask] == 4).all() and got[2].max() > 4
    ctx.set_option("chunk_spp", 2)   # spp_min is reached in the tile's second chunk: the first item still writes ns = spp_min
    ctx.set_option("chunk_tail", 3)
    assert same(three_ways(ctx, blobs, "box", WIDE, region, 4, spp_max=16), got)


def test_coloured_background(ctx, blobs):
    region = (0, 0) + SMALL
    got = three_ways(ctx, blobs, "coloured_background", SMALL, region, 8)
    mask = ctx.empty_tiles(region)
    assert mask.any() and background_tiles(blobs("coloured_background", SMALL), got, 8, SMALL)[mask].all()
    assert np.array_equal(background_of(blobs("coloured_background", SMALL)), np.array([0.25, 0.5, 0.125], np.float32))


@pytest.mark.parametrize("name", ["far_spheres", "tilted_plane", "nested_groups"])
def test_scenes(ctx, blobs, name):
    region = (0, 0) + SMALL
    got = three_ways(ctx, blobs, name, SMALL, region, 8)
    mask = ctx.empty_tiles(region)
    assert mask.any() and not mask.all()
    assert background_tiles(blobs(name, SMALL), got, 8, SMALL)[mask].all()


@pytest.mark.parametrize("name", ["depth_of_field", "camera_inside"])
def test_no_empty_tile(ctx, blobs, name):
    region = (0, 0) + SMALL
    three_ways(ctx, blobs, name, SMALL, region, 8)
    assert not ctx.empty_tiles(region).any()


def test_nan_background(ctx, blobs):
    """No tile is empty, and the option changes nothing (a NaN has no bits to compare with the oracle's: on against off)."""
    from empty_tile_util import nan_background
    ctx.upload_scene(nan_background(blobs("box", SMALL).copy()))
    region = (0, 0) + SMALL
    assert not ctx.empty_tiles(region).any()
    on_and_off(ctx, lambda c: c.render_region(region, 8))


def test_progressive_frame(ctx, blobs):
    """Four passes of 4 spp: a pass resumes pixels that come with state and keeps the traced path; the finished frame is the
    one-shot frame, which takes the shortcut."""
    region = (0, 0) + WIDE
    one = three_ways(ctx, blobs, "box", WIDE, region, 16)
    ctx.reset_counters()
    with ctx.progressive(region, 16) as prog:
        for s in (4, 8, 12, 16):
            prog.advance(s)
        frame = prog.read()
    assert same(words(frame, ctx.counters()), one)
