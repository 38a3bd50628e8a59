"""The empty-tile test (qaray_amd/csrc/hip/qa_emptytile.h: "no camera ray of this 8x8 tile can hit anything") on the CPU.  The mask
comes from the library's host build of the header (hip.empty_tiles_host); tests/cpp/empty_tile_check.cpp, built stand-alone with
AddressSanitizer + UBSan, puts the rays of every tile called empty to the nodes' first gates as the walk applies them (restated there
from the device-only qa_kernel.h, like tests/cpp/last_cast_check.cpp's intersectors), and the oracle's frame must be background there."""
import numpy as np
import pytest

from conftest import bits
from empty_tile_util import NO_EMPTY_TILE, SCENES, background_of, nan_background, scene_blob, tile_all
from test_cast_cost_host import build, fields

WIDE = (192, 64)
SPP = 4


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    return build(tmp_path_factory, "empty_tile_check")


def frame_line(out):
    (line,) = [ln for ln in out.splitlines() if " frame=" in ln]
    return fields(line)


def background_tiles(blob, size, spp=SPP):
    """The oracle's frame -> bool [ty, tx]: every pixel of the tile has rgb = the background's bits, depth = QA_BIGFLOAT, ns = spp."""
    from oracle import binding as oracle
    rgb, depth, ns, _ = oracle.render(blob, (0, 0) + size, spp)
    bg = bits(background_of(blob))
    pure = (bits(rgb) == bg).all(axis=2) & (bits(depth) == bits(np.float32(1.0e30))) & (ns == spp)
    return tile_all(pure, size)


def test_flagship_frame(check, tmp_path):
    """The Cornell box at 1920x1080: every tile called empty is pure background in the oracle's frame, and at least 13 000 of the
    32 400 tiles are called empty (the oracle alone finds 13 553 whose eight neighbours are background too; the test's half-pixel
    margin and slack may lose the ring next to the box and nothing more)."""
    from qaray_amd import hip
    from qaray_amd.host import load_scene_blob
    size = (1920, 1080)
    blob = load_scene_blob("example_project12_box.xml", size=size)
    mask = hip.empty_tiles_host(blob, (0, 0) + size)
    assert mask.shape == (135, 240)
    pure = background_tiles(blob, size)
    print(f"tiles called empty: {int(mask.sum())}; pure background in the oracle's frame: {int(pure.sum())}")
    assert not (mask & ~pure).any(), np.argwhere(mask & ~pure)[:5]
    assert int(mask.sum()) >= 13000
    p = str(tmp_path / "box_1080p.bin")
    blob.tofile(p)
    f = frame_line(check("rays", "24", p))
    assert f["passed"] == "0" and int(f["empty"]) == int(mask.sum()) and f["variant"] == "1", f


@pytest.mark.parametrize("name", sorted(SCENES))
def test_scenes_ray_by_ray(check, tmp_path, name):
    """A few hundred sample positions and the four corners of every tile called empty: every node's first gate turns them away.  The
    mask is the library's, the scene still runs on the last-cast variant, and the oracle's frame is background in those tiles."""
    from qaray_amd import hip
    blob = scene_blob(tmp_path, name, WIDE)
    p = str(tmp_path / f"{name}.bin")
    blob.tofile(p)
    out = check("rays", "300", p)
    print(out)
    f = frame_line(out)
    mask = hip.empty_tiles_host(blob, (0, 0) + WIDE)
    assert f["passed"] == "0" and f["variant"] == "1" and int(f["tiles"]) == mask.size, f
    if name == "depth_of_field":   # the header's test knows no lens; the launch's rule (no tile lists with depth of field) is the library's
        assert not mask.any()
        return
    assert int(f["empty"]) == int(mask.sum()), f
    assert (int(f["empty"]) == 0) == (name in NO_EMPTY_TILE), f
    pure = background_tiles(blob, WIDE)
    assert not (mask & ~pure).any(), np.argwhere(mask & ~pure)[:5]
    if name not in NO_EMPTY_TILE:
        assert int(f["rays"]) == 304 * int(f["empty"]) and not mask.all(), f


def test_far_spheres_are_seen(tmp_path):
    """The two spheres of radius 0.01 stand beside the box, one on either side: each takes tiles out of the box scene's mask, and
    neither takes them all (the slack grows with the square of the origin's distance; it is no blanket "never empty")."""
    from qaray_amd import hip
    blob = scene_blob(tmp_path, "far_spheres", WIDE)
    mask = hip.empty_tiles_host(blob, (0, 0) + WIDE)
    box = hip.empty_tiles_host(scene_blob(tmp_path, "box", WIDE), (0, 0) + WIDE)
    lost = box & ~mask
    assert lost.any() and not (mask & ~box).any()
    half = WIDE[0] // 16
    assert lost[:, :half].any() and lost[:, half:].any()
    assert mask[:, :half].any() and mask[:, half:].any()


def test_nan_background(check, tmp_path):
    from qaray_amd import hip
    blob = nan_background(scene_blob(tmp_path, "box", WIDE))
    assert not hip.empty_tiles_host(blob, (0, 0) + WIDE).any()
    p = str(tmp_path / "nan.bin")
    blob.tofile(p)
    f = frame_line(check("rays", "4", p))
    assert f["empty"] == "0" and f["variant"] == "1", f


def test_regions_and_strips(tmp_path):
    """An off-grid region's tiles start at its own corner; strips are rows of the region's mask."""
    from qaray_amd import hip
    blob = scene_blob(tmp_path, "box", WIDE)
    region = (5, 3, 187, 61)
    whole = hip.empty_tiles_host(blob, region)
    assert whole.shape == (8, 23) and whole.any() and not whole.all()
    assert np.array_equal(hip.empty_tiles_host(blob, region, 1, 3), whole[1::3])
    with pytest.raises(hip.HipError):
        hip.empty_tiles_host(blob, (0, 0, 200, 64))
