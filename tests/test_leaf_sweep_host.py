"""The leaf sweep of the last-cast query (qa_kernel.h sweepLeaves: a bounce ray of qa_integrate_lastcast tests every box of a small
mesh's leaf table once and then the triangles of its own candidates, instead of walking the own tree), on the CPU:
tests/cpp/leaf_sweep_check.cpp restates it from the headers the kernel uses and puts the query with the sweep, the query with the
walk and the reference's closest-hit sweep to every bounce ray - on the five poses of the Cornell box, on the scenes made to trip
the query, and on meshes that must keep the walk.  Built stand-alone with AddressSanitizer + UBSan."""
import re

import pytest

from last_cast_util import SCENES, scene_blob
from leaf_sweep_util import SCENES as TABLE_SCENES, scene_blob as table_blob
from test_cast_cost_host import build, fields
from tile_list_util import POSES, pose_blob

SIZE = (152, 150)


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    return build(tmp_path_factory, "leaf_sweep_check")


def frame_line(out):
    (line,) = [ln for ln in out.splitlines() if " frame=" in ln]
    return fields(line)


def outcomes_add_up(f):
    return int(f["blocked"]) + int(f["glowHits"]) + int(f["escaped"]) + int(f["again"]) == int(f["bounce"])


@pytest.mark.parametrize("pose", POSES)
def test_sweep_equals_the_reference_sweep_on_the_poses(check, tmp_path, pose):
    """6 camera rays per tile and a bounce ray from every hit: no mismatch in any order of the candidates, and fewer than 1 % of the
    bounce rays ask again (the cap that keeps the fall-back from hiding a broken fast path) - in the shipped order and in every
    other."""
    p = str(tmp_path / f"{pose}.bin")
    pose_blob(pose, SIZE).tofile(p)
    out = check("rays", "6", "fast", p)
    print(out)
    f = frame_line(out)
    assert f["mismatches"] == "0" and f["resident"] == "1", f
    assert f["sweptMeshes"] == "1" and f["walkedMeshes"] == "0" and f["leavesMax"] == "18", f
    assert int(f["bounce"]) > (200 if pose == "partly_behind" else 1500), f
    assert int(f["swept"]) > 0 and int(f["walked"]) == 0, f
    assert 100 * int(f["again"]) < int(f["bounce"]) and 100 * int(f["againMax"]) < int(f["bounce"]), f
    assert outcomes_add_up(f), f
    if pose in ("box", "scaled_rotated"):
        assert int(f["glowHits"]) > 0, f


@pytest.mark.parametrize("name", sorted(SCENES))
def test_sweep_equals_the_reference_sweep_on_scenes_made_to_trip_the_query(check, tmp_path, name):
    p = str(tmp_path / f"{name}.bin")
    scene_blob(tmp_path, name, SIZE).tofile(p)
    out = check("rays", "6", "fast", p)
    print(out)
    f = frame_line(out)
    assert f["mismatches"] == "0" and int(f["bounce"]) > 1500 and f["sweptMeshes"] == "1", f
    assert int(f["glowHits"]) > 0 and int(f["blocked"]) > 0 and int(f["escaped"]) > 0, f   # every outcome of the query is met
    assert 100 * int(f["again"]) < int(f["bounce"]) and 100 * int(f["againMax"]) < int(f["bounce"]), f
    assert outcomes_add_up(f), f


@pytest.mark.parametrize("pose", ("box", "scaled_rotated"))
def test_a_zero_direction_component_in_the_wave(check, tmp_path, pose):
    """Every eighth bounce ray has a direction component of exactly zero, and every ray takes the exact slab form, as the lanes of
    a wave with such a ray do (the wave-uniform !fastSlab)."""
    p = str(tmp_path / f"{pose}.bin")
    pose_blob(pose, SIZE).tofile(p)
    out = check("rays", "6", "slow", p)
    print(out)
    f = frame_line(out)
    assert f["mismatches"] == "0" and f["form"] == "slow" and int(f["bounce"]) > 1500 and int(f["swept"]) > 1500, f
    assert 100 * int(f["again"]) < int(f["bounce"]) and outcomes_add_up(f), f


def test_a_tree_of_one_leaf_keeps_the_walk(check, tmp_path):
    """The box and a floor of two triangles: the box is swept, the floor's own tree is its root leaf - no box to test."""
    p = str(tmp_path / "one_leaf.bin")
    table_blob(tmp_path, "one_leaf", SIZE).tofile(p)
    out = check("rays", "16", "fast", p)
    print(out)
    f = frame_line(out)
    assert f["mismatches"] == "0" and f["resident"] == "1" and f["sweptMeshes"] == "1" and f["walkedMeshes"] == "1", f
    assert int(f["swept"]) > 500 and int(f["walked"]) > 500 and outcomes_add_up(f), f
    assert int(f["glowHits"]) > 0 and int(f["blocked"]) > 0 and int(f["escaped"]) > 0, f


def test_a_tree_of_more_leaves_than_a_table_holds_keeps_the_walk(check, tmp_path):
    """70 leaves: the mesh has no leaf table (QA_TILE_LEAF_CAP = 64) and the query walks its tree, as it walks the one-leaf ground's:
    rays, counts and answers are the walk's."""
    assert sorted(TABLE_SCENES) == ["many_leaves", "one_leaf"]
    p = str(tmp_path / "many_leaves.bin")
    table_blob(tmp_path, "many_leaves", SIZE).tofile(p)
    out = check("rays", "16", "fast", p)
    print(out)
    f = frame_line(out)
    assert f["mismatches"] == "0" and f["resident"] == "1" and f["sweptMeshes"] == "0" and f["walkedMeshes"] == "2" and f["leavesMax"] == "1", f
    assert int(f["swept"]) == 0 and int(f["walked"]) > 500 and outcomes_add_up(f), f
    assert f["again"] == f["againWalk"] == f["againMax"], f
    assert int(f["glowHits"]) > 0 and int(f["blocked"]) > 0 and int(f["escaped"]) > 0, f


def test_the_sorted_table_is_the_leaf_table_largest_box_first(check, tmp_path):
    """The model's `area` form reads the table the host sorted; `table` the leaf table.  Both hold the same 18 records: the same box
    tests per ray, and on the box the sorted one needs fewer triangle tests per tile (why it is the one that ships)."""
    p = str(tmp_path / "box.bin")
    pose_blob("box", SIZE).tofile(p)
    out = check("rays", "64", "fast", p)
    print(out)
    rows = {ln.split()[0]: ln for ln in out.splitlines() if ln.startswith("  ") and "envelope" in ln}
    env = {k: [float(x) for x in re.search(r"tiles\)\s+([\d.]+) (?:box tests|node visits)\s+([\d.]+) triangle tests", rows[k]).groups()] for k in rows}
    # [box tests | node visits, triangle tests] of the slowest ray of a tile
    assert env["table"][0] == env["area"][0] == 18.0, env
    assert env["area"][1] < env["table"][1] < env["walk"][1], env
    est = {k: float(rows[k].split("estimate")[1].split()[0]) for k in rows}
    assert est["area"] < 0.8 * est["walk"], est   # the stop rule: at least 20 % fewer issued instructions than the walk
