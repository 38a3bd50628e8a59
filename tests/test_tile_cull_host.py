"""The per-tile leaf lists of camera rays (qaray_amd/csrc/hip/qa_tilecull.h) on the CPU: tests/cpp/tile_cull_check.cpp, built
with AddressSanitizer + UBSan like the scene builder's check (tests/test_sanitizers.py), draws 256 random sub-pixel camera rays
per tile and requires every leaf whose widened box passes the walk's own test to be on the tile's list - no omission allowed."""
import os
import re
import subprocess

import pytest

from conftest import ROOT
from tile_list_util import POSES, pose_blob

SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    hip = os.path.join(ROOT, "qaray_amd", "csrc", "hip")
    exe = str(tmp_path_factory.mktemp("tile_cull") / "tile_cull_check")
    subprocess.run(["g++", "-std=c++17", *SAN, "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{ROOT}/include",
                    f"-I{hip}", os.path.join(ROOT, "tests", "cpp", "tile_cull_check.cpp"), os.path.join(hip, "qa_scene_build.cpp"), "-o", exe],
                   check=True)

    def run(*args):
        r = subprocess.run([exe, *args], env=ENV, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0 and "tile_cull_check: clean" in r.stdout, r.stdout[-3000:]
        assert "runtime error" not in r.stdout and "AddressSanitizer" not in r.stdout, r.stdout[-3000:]
        return r.stdout
    return run


def fields(line):
    return {k: v for k, v in re.findall(r"(\w+)=([\w.]+)", line)}


# what each pose must be for the check to mean something: (origin inside the mesh bounds, inside a leaf box, corners of the bounds behind the camera)
EXPECT = {"box": (0, 0, "none"), "scaled_rotated": (0, 0, "none"), "origin_in_bounds": (1, 0, "some"), "origin_in_leaf": (1, 1, "some"),
          "partly_behind": (0, 0, "some")}


@pytest.mark.parametrize("pose", POSES)
def test_no_leaf_is_missing_from_a_tile_list(check, tmp_path, pose):
    paths = []
    for size in ((152, 150), (61, 45)):
        p = str(tmp_path / f"{pose}_{size[0]}x{size[1]}.bin")
        pose_blob(pose, size).tofile(p)
        paths.append(p)
    lines = [ln for ln in check("rays", *paths).splitlines() if " node=" in ln]
    assert len(lines) == 2, lines
    for ln in lines:
        f = fields(ln)
        assert f["omissions"] == "0" and int(f["required"]) > 0 and int(f["leaves"]) == 18, ln
        in_bounds, in_leaf, behind = EXPECT[pose]
        assert int(f["originInBounds"]) == in_bounds and (int(f["originInLeaves"]) > 0) == bool(in_leaf), ln
        assert (0 < int(f["cornersBehind"]) < 8) == (behind == "some"), ln


def test_list_lengths_of_the_flagship_frame(check, tmp_path):
    """The Cornell box at 1920x1080 (BASELINE C2): the histogram recorded in profiles/tile_lists.txt."""
    p = str(tmp_path / "box_1080p.bin")
    pose_blob("box", (1920, 1080)).tofile(p)
    out = check("hist", p)
    m = re.search(r"listed per such tile: ([\d.]+) leaves, ([\d.]+) triangles", out)
    assert m, out
    print(out)
    # the cost model the path was built on: lists of 2 - 4 leaves, 4 - 8 triangle tests, against a walk's 8.7 node visits and 2.7 tests
    assert float(m.group(1)) <= 4.0 and float(m.group(2)) <= 8.0, out
    assert "+ 480 B of tile lists" in out and "dynamic LDS 31520 B" in out, out   # 32 000 B: 25 units of 1280 B, five workgroups per CU
