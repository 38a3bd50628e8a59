"""The triangle phase of the last-cast query's leaf sweep, a leaf per turn (qa_kernel.h sweepLeaves: a lane reads
where its candidate leaf's triangles are from one byte in LDS and tests both in straight-line code), on the CPU:
tests/cpp/leaf_pair_check.cpp restates that loop and the one it replaced (one triangle per turn, the sweep as commit 55d1672's
parent had it: the specification) from the headers the kernel uses and puts both to every
bounce ray - on the five poses of the Cornell box, on the scenes made to trip the query, on a mesh of an odd triangle count and
on meshes that keep the walk - and checks the byte table the scene builder writes.  Built stand-alone with AddressSanitizer +
UBSan."""
import pytest

from last_cast_util import SCENES, scene_blob
from leaf_pair_util import odd_floor_blob
from leaf_sweep_util import scene_blob as table_blob
from test_cast_cost_host import build, fields
from tile_list_util import POSES, pose_blob

SIZE = (152, 150)


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    return build(tmp_path_factory, "leaf_pair_check")


def frame_line(out):
    (line,) = [ln for ln in out.splitlines() if " frame=" in ln]
    return {k: (v if k == "frame" else int(v)) for k, v in fields(line).items()}


def same_answers(f):
    assert f["mismatches"] == 0 and f["outside"] == 0 and f["tableErrors"] == 0, f


def test_the_byte_table_of_made_up_leaves(check):
    out = check("bytes")
    print(out)
    assert "WRONG" not in out and out.count(" ok\n") == 6, out


@pytest.mark.parametrize("pose", POSES)
def test_pair_equals_single_on_the_poses(check, tmp_path, pose):
    """6 camera rays per tile, a bounce ray from every hit, and every accepted ray once more at exactly its distance: the same hit,
    best, tie and hz from both loops.  The box's 18 leaves hold two triangles each."""
    p = str(tmp_path / f"{pose}.bin")
    pose_blob(pose, SIZE).tofile(p)
    out = check("rays", "6", p)
    print(out)
    f = frame_line(out)
    same_answers(f)
    assert f["meshes"] == 1 and f["tables"] == 1 and f["oneTriLeaves"] == 0 and f["lastRecordLeaves"] == 1, f
    assert f["bounce"] > (200 if pose == "partly_behind" else 1500) and f["walked"] == 0, f
    assert f["queries"] == f["bounce"] + f["atTie"] and f["ties"] >= f["atTie"], f   # every ray asked again at its own distance met that tie
    assert f["pairTurns"] < f["singleTurns"], f
    if pose != "partly_behind":   # (that camera sees the box from outside: nearly all of its bounce rays leave the scene)
        assert f["atTie"] > 0.5 * f["bounce"], f
        assert 0 < f["second"] < f["hits"], f       # some accepted triangle is its leaf's second one


@pytest.mark.parametrize("name", ("coplanar_after", "coplanar_before"))
def test_pair_equals_single_on_the_coplanar_scenes(check, tmp_path, name):
    assert name in SCENES
    p = str(tmp_path / f"{name}.bin")
    scene_blob(tmp_path, name, SIZE).tofile(p)
    out = check("rays", "6", p)
    print(out)
    f = frame_line(out)
    same_answers(f)
    assert f["tables"] == 1 and f["bounce"] > 1500 and f["hits"] > 0 and f["ties"] > 0 and f["second"] > 0, f


def test_a_mesh_of_an_odd_triangle_count(check, tmp_path):
    """The box and a floor of five triangles, both swept: the floor's own tree has a leaf of one triangle (the pair form reads that
    record twice) and a leaf that ends at the mesh's last record; no index leaves the mesh's records."""
    p = str(tmp_path / "odd_floor.bin")
    odd_floor_blob(tmp_path, SIZE).tofile(p)
    out = check("rays", "16", p)
    print(out)
    f = frame_line(out)
    same_answers(f)
    assert f["meshes"] == 2 and f["tables"] == 2 and f["noTable"] == 0, f
    assert f["oneTriLeaves"] >= 1 and f["lastRecordLeaves"] == 2, f
    assert f["oneTriTurns"] > 0 and f["hits"] > 500 and f["walked"] == 0, f


def test_a_one_leaf_mesh_has_no_table(check, tmp_path):
    """The box and a floor of two triangles: the box is swept a leaf per turn; the floor's own tree is one leaf, and a tree of one
    leaf keeps the walk whatever its bytes say."""
    p = str(tmp_path / "one_leaf.bin")
    table_blob(tmp_path, "one_leaf", SIZE).tofile(p)
    out = check("rays", "16", p)
    print(out)
    f = frame_line(out)
    same_answers(f)
    assert f["meshes"] == 2 and f["queries"] > 500 and f["walked"] > 500, f


def test_a_mesh_of_more_than_64_leaves_has_no_table(check, tmp_path):
    """70 leaves: no leaf table, no bytes, leafPairs = 0 - every query of the scene walks."""
    p = str(tmp_path / "many_leaves.bin")
    table_blob(tmp_path, "many_leaves", SIZE).tofile(p)
    out = check("rays", "16", p)
    print(out)
    f = frame_line(out)
    same_answers(f)
    assert f["meshes"] == 2 and f["noTable"] >= 1 and f["queries"] == 0 and f["walked"] > 500, f
