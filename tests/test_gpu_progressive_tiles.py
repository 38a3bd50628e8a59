"""Progressive frames refined tile by tile: passes over a caller's choice of tiles (advance_tiles), the per-tile level and error
maps, and noisiest-first passes (advance_adaptive).

A pass changes when a pixel takes its samples, never which, so every frame here ends bit-identical to the one-shot render_region
frame (and so to the oracle the goldens come from), and counters summed over the passes equal the one-shot frame's: no pass takes
a sample beyond its target.  The device's error map equals the host build of its source (qa_test_tile_error_host) and the numpy
restatement of its specification bit for bit, and an adaptive pass raises exactly the tiles qa_test_tile_select_host predicts from
the maps read before it (tests/test_progressive_tiles_host.py pins both host builds to the restatements)."""
import numpy as np
import pytest

from conftest import bits, ensure_assets, golden_blob, load_golden
from progressive_tiles_util import tile_error_np

pytestmark = pytest.mark.gpu

QA_EINVAL, QA_EUNSUPPORTED = -1, -6
CNT = ("samples", "casts_normal", "casts_shadow", "pixels")
SIZE = (64, 48)
FULL = (0, 0, 64, 48)
REGION = (3, 5, 43, 33)   # 5 x 4 tiles, the last tile row 4 pixel rows high, off the image's own tile grid

# scene, what must run
FAMILIES = {
    "box_lastcast": ("example_project12_box.xml", "LASTCAST=1"),
    "sphere": ("example_project3_sphere.xml", "qa_integrate<"),
    "tower_cs": ("trc_scene_tower.xml", "qa_integrate_cs_resume<"),
    "object_textured": ("example_project7_object.xml", "TEX=1"),
    "area": ("example_project10_test.xml", "AREA=1"),
}


@pytest.fixture(scope="module")
def ctx():
    from qaray_amd import hip
    c = hip.Context(0)
    yield c
    c.set_option("progressive_tile_limit", 0)
    c.close()


def blob(scene):
    from qaray_amd.host import load_scene_blob
    ensure_assets()
    return load_scene_blob(scene, size=SIZE)


def same(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def tile_shape(region):
    return (region[3] - region[1] + 7) // 8, (region[2] - region[0] + 7) // 8


def pixels_of(mask, region):
    """A tile mask as a mask of the region's pixels."""
    h, w = region[3] - region[1], region[2] - region[0]
    return np.kron(mask.astype(np.uint8), np.ones((8, 8), np.uint8))[:h, :w].astype(bool)


def mixed(mask, region, hi, lo):
    """The frame whose selected tiles are `hi`'s and whose other tiles are `lo`'s."""
    p = pixels_of(mask, region)
    return tuple(np.where(p[..., None] if a.ndim == 3 else p, a, b) for a, b in zip(hi, lo))


def checker(region):
    """A checkerboard over the left tile columns and one tile on its own in the right ones."""
    ty, tx = tile_shape(region)
    m = (np.add.outer(np.arange(ty), np.arange(tx)) % 2 == 0)
    m[:, tx - 2:] = False
    m[1, tx - 1] = True
    return m


@pytest.mark.parametrize("case,region", [(c, REGION) for c in sorted(FAMILIES)] + [("box_lastcast", FULL), ("tower_cs", FULL)])
def test_selected_tiles_advance_alone(ctx, case, region):
    """Fixed spp: after advance(4) and advance_tiles(16, mask) the frame is the 16-sample frame on the mask's tiles and the
    4-sample frame elsewhere; advance(16) completes it; the samples of all passes are the one-shot frame's; a device mask does
    what the host mask does."""
    import torch
    scene, kernel = FAMILIES[case]
    ctx.upload_scene(blob(scene))
    ref4 = ctx.render_region(region, 4)
    ctx.reset_counters()
    ref16 = ctx.render_region(region, 16)
    c1 = ctx.counters()
    mask = checker(region)
    ctx.reset_counters()
    with ctx.progressive(region, 16) as prog:
        assert prog.tile_shape == tile_shape(region) == mask.shape
        prog.advance(4)
        prog.advance_tiles(16, mask)
        assert kernel in ctx.kernel_name(), ctx.kernel_name()
        frame = prog.read()
        assert same(frame, mixed(mask, region, ref16, ref4))
        assert np.array_equal(prog.tile_levels(), np.where(mask, 16, 4))
        st = prog.status()
        assert st["tiles_behind"] == int((~mask).sum()) and st["spp_reached"] == 4
        assert st["pixels_finished"] == int(pixels_of(mask, region).sum())
        prog.advance(16)
        assert same(prog.read(), ref16)
        assert prog.status() == {"spp_reached": 16, "tiles_behind": 0, "pixels_finished": frame[2].size}
        c2 = ctx.counters()
        assert all(c1[k] == c2[k] for k in CNT), (c1, c2)
        # the same with the mask in device memory (uint8), on a fresh frame
        prog.restart()
        prog.advance(4)
        d_mask = torch.from_numpy(mask.astype(np.uint8)).to(f"cuda:{ctx.device_id}")
        prog.advance_tiles(16, d_mask)
        assert same(prog.read(), frame)
        levels = prog.tile_levels_device()
        ctx.synchronize()
        assert levels.dtype == torch.int32 and np.array_equal(levels.cpu().numpy(), np.where(mask, 16, 4))


def live_level(levels, error):
    """The lowest level among the tiles that still have something to gain (error > 0); None when there is none."""
    live = error > 0
    return int(levels[live].min()) if live.any() else None


@pytest.mark.parametrize("region", [None, REGION])
def test_noisiest_first_passes_build_the_golden_frame(ctx, region):
    """sphere_adaptive_64x48_4to32spp in noisiest-quarter passes: advance(4), then advance_adaptive(min(level + 8, spp_max),
    fraction=0.25) until a pass selects nothing, `level` being the lowest level among the tiles whose error is not 0 (a tile whose
    pixels all finished keeps its level for good and can gain nothing).  Every pass raises exactly the tiles qa_test_tile_select_host
    picks from the maps read before it and changes no other pixel; the finished frame is the golden's and the one-shot frame's.
    Levels move on the ladder 4, 12, 20, 28, 32 and every selecting pass raises at least one tile one step: a finished frame cannot
    take more than 4 * tiles such passes."""
    from qaray_amd import hip
    rgb, depth, ns, meta = load_golden("sphere_adaptive_64x48_4to32spp")
    ctx.upload_scene(golden_blob(meta))
    golden = region is None
    region = tuple(meta["crop"]) if golden else region
    args = dict(max_bounce=meta["bounce"], seed=meta["seed"], spp_max=meta["spp_max"])
    ty, tx = tile_shape(region)
    quarter = -(-ty * tx // 4)
    passes = 0
    with ctx.progressive(region, meta["spp_min"], **args) as prog:
        assert prog.adaptive_info() == {"selected": 0, "candidates": 0, "cut_error": 0.0, "max_finite_error": 0.0}
        prog.advance(4)
        while True:
            levels, error, before = prog.tile_levels(), prog.tile_error(), prog.read()
            low = live_level(levels, error)
            target = min((low if low is not None else int(levels.min())) + 8, meta["spp_max"])
            want, want_info = hip.tile_select_host(error, levels, target, quarter)
            prog.advance_adaptive(target, fraction=0.25)
            info = prog.adaptive_info()
            after_levels, after = prog.tile_levels(), prog.read()
            assert info["selected"] == want_info["selected"] == int(want.sum()) and info["candidates"] == want_info["candidates"]
            assert np.float32(info["cut_error"]).view(np.uint32) == want_info["cut_bits"]
            assert np.float32(info["max_finite_error"]).view(np.uint32) == want_info["max_finite_bits"]
            assert np.array_equal(after_levels > levels, want) and (after_levels[want] == target).all()
            assert np.array_equal(after_levels[~want], levels[~want])
            keep = ~pixels_of(want, region)
            assert all(np.array_equal(bits(a)[keep], bits(b)[keep]) for a, b in zip(after, before))
            if info["selected"] == 0:
                break
            passes += 1
            assert passes <= 4 * ty * tx
        assert low is None and passes >= 4   # nothing left to gain, and it took several passes to get there
        frame = prog.read()
        assert prog.status()["pixels_finished"] == frame[2].size
    one = ctx.render_region(region, meta["spp_min"], **args)
    assert same(frame, one)
    if golden:
        assert np.array_equal(frame[2], ns) and np.array_equal(bits(frame[1]), bits(depth))


@pytest.mark.parametrize("case,region", [("sphere", REGION), ("tower_cs", FULL), ("box_lastcast", REGION)])
def test_error_map_is_the_host_build_s(ctx, case, region):
    """spp 2 .. 32: after passes to 1, 2 and 9 the device's error map is the host build's of the frame's state and the numpy
    restatement's, bit for bit; +inf everywhere at level 1 (no pixel has a variance yet); 0 on tiles whose pixels all finished."""
    import torch
    from qaray_amd import hip
    scene, kernel = FAMILIES[case]
    ctx.upload_scene(blob(scene))
    with ctx.progressive(region, 2, spp_max=32) as prog:
        for s in (1, 2, 9):
            prog.advance(s)
            state, error = prog.state(), prog.tile_error()
            assert kernel in ctx.kernel_name(), ctx.kernel_name()
            assert state.shape == (region[3] - region[1], region[2] - region[0], 8) and error.shape == tile_shape(region)
            assert np.array_equal(bits(error), bits(hip.tile_error_host(state))), (case, s)
            assert np.array_equal(bits(error), bits(tile_error_np(state))), (case, s)
            finished = (state[..., 1] >> 31) == 1
            assert np.array_equal(state[..., 1][~finished], np.full(int((~finished).sum()), s, np.uint32))
            done = np.array([[finished[8 * j:8 * j + 8, 8 * i:8 * i + 8].all() for i in range(error.shape[1])] for j in range(error.shape[0])])
            assert (bits(error)[done] == 0).all() and (error[~done] > 0).all()
            if s == 1:
                assert np.isposinf(error).all() and not finished.any()
            else:
                assert np.isfinite(error).all()
            d_error = prog.tile_error_device()
            ctx.synchronize()
            assert d_error.dtype == torch.float32 and np.array_equal(bits(d_error.cpu().numpy()), bits(error))


def test_torn_selective_and_adaptive_passes_complete_without_overshoot(ctx):
    """progressive_tile_limit ends a pass after n tiles as a stop would: a torn selective pass and a torn adaptive pass leave
    tiles of their choice behind, re-issued passes complete them, and the counters of all passes are the one-shot frame's."""
    ctx.upload_scene(blob("example_project3_sphere.xml"))
    region = REGION
    ty, tx = tile_shape(region)
    ctx.reset_counters()
    one = ctx.render_region(region, 4, spp_max=32)
    c1 = ctx.counters()
    mask = checker(region)
    chosen = int(mask.sum())
    assert chosen == 7
    ctx.reset_counters()
    try:
        with ctx.progressive(region, 4, spp_max=32) as prog:
            prog.advance(4)
            ctx.set_option("progressive_tile_limit", 3)
            prog.advance_tiles(16, mask)
            lv = prog.tile_levels()
            assert (lv == 16).sum() == 3 and (lv[~mask] == 4).all() and prog.status()["tiles_behind"] == ty * tx - 3
            prog.advance_tiles(16, mask)
            lv = prog.tile_levels()
            assert (lv == 16).sum() == 6 and (lv[~mask] == 4).all()
            prog.advance_tiles(16, mask)   # the one tile left of the choice, not two more
            assert np.array_equal(prog.tile_levels(), np.where(mask, 16, 4))
            # an adaptive pass torn after 2 of its 5 tiles
            ctx.set_option("progressive_tile_limit", 2)
            before = prog.tile_levels()
            prog.advance_adaptive(24, max_tiles=5)
            info, lv = prog.adaptive_info(), prog.tile_levels()
            assert info["selected"] == 5 and (lv != before).sum() == 2 and (lv[lv != before] == 24).all()
            ctx.set_option("progressive_tile_limit", 0)
            prog.advance_adaptive(24)      # every tile with something to gain
            lv = prog.tile_levels()
            assert prog.adaptive_info()["selected"] == int((lv == 24).sum()) - 2
            assert (prog.tile_error()[lv < 24] == 0).all()
            prog.advance(32)
            frame = prog.read()
            assert prog.status()["pixels_finished"] == frame[2].size
    finally:
        ctx.set_option("progressive_tile_limit", 0)
    c2 = ctx.counters()
    assert same(frame, one)
    assert all(c1[k] == c2[k] for k in CNT), (c1, c2)


def test_a_frame_of_more_tiles_than_one_turn_of_the_selection_kernels(ctx):
    """66 x 65 = 4290 tiles: qa_prog_select_mask walks 4096 places a turn and qa_prog_adaptive_mask 1024 tiles a turn, so both take
    several turns here, with ties and the cut falling inside them.  A random mask, then the 1500 noisiest tiles, then the rest."""
    from qaray_amd import hip
    from qaray_amd.host import load_scene_blob
    ensure_assets()
    size = (528, 520)
    region = (0, 0) + size
    ctx.upload_scene(load_scene_blob("example_project12_box.xml", size=size))   # (noisy nearly everywhere: thousands of candidates)
    ctx.reset_counters()
    one = ctx.render_region(region, 2, spp_max=6)
    c1 = ctx.counters()
    ty, tx = tile_shape(region)
    assert ty * tx == 4290
    mask = np.random.default_rng(3).random((ty, tx)) < 0.4
    ctx.reset_counters()
    with ctx.progressive(region, 2, spp_max=6) as prog:
        prog.advance(2)
        prog.advance_tiles(4, mask)
        levels = prog.tile_levels()
        assert np.array_equal(levels, np.where(mask, 4, 2)) and prog.status()["tiles_behind"] == int((~mask).sum())
        error = prog.tile_error()
        assert np.array_equal(bits(error), bits(hip.tile_error_host(prog.state())))
        want, want_info = hip.tile_select_host(error, levels, 6, 1500)
        assert want_info["selected"] == 1500 < want_info["candidates"]
        prog.advance_adaptive(6, max_tiles=1500)
        info = prog.adaptive_info()
        assert (info["selected"], info["candidates"]) == (1500, want_info["candidates"])
        assert np.float32(info["cut_error"]).view(np.uint32) == want_info["cut_bits"]
        assert np.array_equal(prog.tile_levels(), np.where(want, 6, levels))
        prog.advance(6)
        frame = prog.read()
        assert prog.status() == {"spp_reached": 6, "tiles_behind": 0, "pixels_finished": size[0] * size[1]}
    c2 = ctx.counters()
    assert same(frame, one)
    assert all(c1[k] == c2[k] for k in CNT), (c1, c2)


def test_refusals_and_lifetime():
    import torch
    from qaray_amd import hip
    c = hip.Context(0)
    try:
        c.upload_scene(blob("example_project3_sphere.xml"))
        ty, tx = tile_shape(REGION)
        every = np.ones((ty, tx), bool)
        # no frame
        ghost = hip.Progressive(c, REGION)
        for call in (lambda: ghost.advance_tiles(4, every), lambda: ghost.advance_adaptive(4), ghost.tile_levels, ghost.tile_error, ghost.state,
                     ghost.adaptive_info):
            with pytest.raises(hip.HipError) as e:
                call()
            assert e.value.code == QA_EINVAL and "qa_progressive_begin" in str(e.value)
        # a frame without variance: no error map, no adaptive pass; levels and selective passes work
        ref = {s: c.render_region(REGION, s) for s in (2, 8)}
        with c.progressive(REGION, 8) as prog:
            prog.advance(2)
            for call in (prog.tile_error, prog.tile_error_device, lambda: prog.advance_adaptive(8)):
                with pytest.raises(hip.HipError) as e:
                    call()
                assert e.value.code == QA_EUNSUPPORTED and "spp_min < spp_max" in str(e.value)
            assert (prog.tile_levels() == 2).all() and same(prog.read(), ref[2])
            # arguments the binding refuses before the library sees them
            for bad, err in ((np.ones((ty, tx + 1), bool), ValueError), (np.ones((ty, tx), np.float32), TypeError), (np.ones(ty * tx, np.uint8), ValueError),
                             (torch.ones((ty, tx), dtype=torch.uint8), ValueError),
                             (torch.ones((ty, tx), dtype=torch.int32, device="cuda:0"), ValueError),
                             (torch.ones((tx, ty), dtype=torch.uint8, device="cuda:0").t(), ValueError)):
                with pytest.raises(err):
                    prog.advance_tiles(8, bad)
            with pytest.raises(ValueError):
                prog.tile_levels_device(out=torch.zeros((ty, tx), dtype=torch.float32, device="cuda:0"))
            with pytest.raises(ValueError):
                prog.advance_adaptive(8, max_tiles=3, fraction=0.5)
            with pytest.raises(ValueError):
                prog.advance_adaptive(8, min_error=-1.0)
            # a null mask, a bad target
            assert hip.lib().qa_progressive_advance_tiles(c._h, 8, None, None) == QA_EINVAL
            assert hip.lib().qa_progressive_advance_tiles_device(c._h, 8, None, None) == QA_EINVAL
            with pytest.raises(hip.HipError) as e:
                prog.advance_tiles(0, every)
            assert e.value.code == QA_EINVAL
            assert same(prog.read(), ref[2])
            # an empty choice takes no sample and changes no pixel
            c.reset_counters()
            prog.advance_tiles(8, np.zeros((ty, tx), np.uint8))
            assert same(prog.read(), ref[2]) and c.counters()["samples"] == 0 and (prog.tile_levels() == 2).all()
            assert prog.status()["tiles_behind"] == ty * tx
            # a one-shot frame between passes disturbs nothing
            half = np.zeros((ty, tx), bool)
            half[:, :2] = True
            prog.advance_tiles(8, half)
            assert same(c.render_region(REGION, 8), ref[8])
            assert same(prog.read(), mixed(half, REGION, ref[8], ref[2]))
            prog.advance_tiles(100, ~half)   # (the target is cut to spp_max)
            assert same(prog.read(), ref[8]) and prog.status()["tiles_behind"] == 0
        # a stale frame: refused until restart()
        with c.progressive(REGION, 2, spp_max=8) as prog:
            prog.advance(2)
            lights = hip.blob_table(c.download_scene(), "lights")
            c.edit_lights(0, lights[:1])
            for call in (lambda: prog.advance_tiles(8, every), lambda: prog.advance_adaptive(8)):
                with pytest.raises(hip.HipError) as e:
                    call()
                assert e.value.code == QA_EINVAL and "restart" in str(e.value)
            assert (prog.tile_levels() == 2).all()   # (the maps still serve the old frame)
            prog.restart()
            prog.advance_tiles(8, every)
            assert same(prog.read(), c.render_region(REGION, 2, spp_max=8))
    finally:
        c.close()
