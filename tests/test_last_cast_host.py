"""The last cast of a path in a resident scene without lights, asked as "which emitter does this ray meet" (qa_kernel.h
lastCastQuery), on the CPU: tests/cpp/last_cast_check.cpp restates the query and the reference's closest-hit sweep and puts
both to every bounce ray - on the five poses of the Cornell box and on scenes made to trip the query - and the scene predicate
(qa_scene_build.cpp PlanLastCast) on built scenes.  Built stand-alone with AddressSanitizer + UBSan."""
import pytest

from last_cast_util import SCENES, SPOILED, scene_blob, spoil
from test_cast_cost_host import build, fields
from tile_list_util import POSES, pose_blob

SIZE = (152, 150)


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    return build(tmp_path_factory, "last_cast_check")


def frame_line(out):
    (line,) = [ln for ln in out.splitlines() if " frame=" in ln]
    return fields(line)


@pytest.mark.parametrize("pose", POSES)
def test_query_equals_the_reference_sweep_on_the_poses(check, tmp_path, pose):
    """6 camera rays per tile and a bounce ray from every hit: no mismatch, and fewer than 1 % of the bounce rays ask again (the cap
    that keeps the fall-back from hiding a broken fast path)."""
    p = str(tmp_path / f"{pose}.bin")
    pose_blob(pose, SIZE).tofile(p)
    out = check("rays", "6", p)
    print(out)
    f = frame_line(out)
    assert f["mismatches"] == "0", f
    assert int(f["bounce"]) > (200 if pose == "partly_behind" else 1500), f
    assert 100 * int(f["again"]) < int(f["bounce"]), f
    assert int(f["blocked"]) + int(f["glowHits"]) + int(f["escaped"]) + int(f["again"]) == int(f["bounce"]), f
    if pose in ("box", "scaled_rotated"):
        assert int(f["glowHits"]) > 0, f


@pytest.mark.parametrize("name", sorted(SCENES))
def test_query_equals_the_reference_sweep_on_scenes_made_to_trip_it(check, tmp_path, name):
    p = str(tmp_path / f"{name}.bin")
    scene_blob(tmp_path, name, SIZE).tofile(p)
    out = check("rays", "6", p)
    print(out)
    f = frame_line(out)
    assert f["mismatches"] == "0" and int(f["bounce"]) > 1500, f
    assert int(f["glowHits"]) > 0 and int(f["blocked"]) > 0 and int(f["escaped"]) > 0, f   # every outcome of the query is met
    assert int(f["glowMask"]) not in (0,), f
    if name == "glow_sphere_and_plane":
        assert bin(int(f["glowMask"])).count("1") == 2, f


def predicate(check, path):
    (line,) = [ln for ln in check("predicate", path).splitlines() if "lastCastQuery=" in ln]
    return fields(line)


def test_predicate_on_built_scenes(check, tmp_path):
    p = str(tmp_path / "box.bin")
    pose_blob("box", SIZE).tofile(p)
    f = predicate(check, p)
    assert f["lastCastQuery"] == "1" and f["glowMask"] == "4" and f["resident"] == "1", f   # node 2: lightPlane
    for how in SPOILED:
        spoil(pose_blob("box", SIZE), how).tofile(p)
        f = predicate(check, p)
        assert f["lastCastQuery"] == "0" and f["glowMask"] == "0", (how, f)
