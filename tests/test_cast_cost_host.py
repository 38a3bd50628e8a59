"""The two shortcuts of a cast on an LDS-resident mesh, on the CPU (qaray_amd/csrc/hip/qa_tilecull.h, qa_kernel.h hitMesh):
tests/cpp/reach_rule_check.cpp - the leaf test that trusts the own tree's answer at the found distance (entry <= t) never trusts
an answer the reference's walk would not give - and tests/cpp/slab_form_check.cpp - the own tree's slab step in its fma form
passes every box the analysis in the header says it must, and the tile lists still hold every leaf it passes.  Both are built
with AddressSanitizer + UBSan like tests/test_tile_cull_host.py's program."""
import os
import re
import subprocess

import pytest

from conftest import ROOT
from tile_list_util import POSES, pose_blob

SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def build(tmp_path_factory, name):
    hip = os.path.join(ROOT, "qaray_amd", "csrc", "hip")
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.run(["g++", "-std=c++17", *SAN, "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{ROOT}/include",
                    f"-I{hip}", os.path.join(ROOT, "tests", "cpp", name + ".cpp"), os.path.join(hip, "qa_scene_build.cpp"), "-o", exe],
                   check=True)

    def run(*args):
        r = subprocess.run([exe, *args], env=ENV, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0 and name + ": clean" in r.stdout, r.stdout[-3000:]
        assert "runtime error" not in r.stdout and "AddressSanitizer" not in r.stdout, r.stdout[-3000:]
        return r.stdout
    return run


@pytest.fixture(scope="module")
def reach(tmp_path_factory):
    return build(tmp_path_factory, "reach_rule_check")


@pytest.fixture(scope="module")
def slab(tmp_path_factory):
    return build(tmp_path_factory, "slab_form_check")


@pytest.fixture(scope="module")
def pose_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("poses")
    out = {}
    for pose in POSES:
        for size in ((152, 150), (61, 45)):
            p = str(d / f"{pose}_{size[0]}x{size[1]}.bin")
            pose_blob(pose, size).tofile(p)
            out[pose, size] = p
    return out


def fields(line):
    return {k: v for k, v in re.findall(r"(\w+)=([\w.]+)", line)}


def node_lines(out):
    return [fields(ln) for ln in out.splitlines() if " node=" in ln]


@pytest.mark.parametrize("pose", POSES)
def test_a_trusted_answer_is_the_reference_walks(reach, pose_files, pose):
    """16 camera rays per tile and a bounce ray from every hit: where entry <= t trusts the own tree's closest triangle and no
    second triangle shares its distance, the reference's walk returns that element at that distance, bit for bit.  (Beside the
    box the camera sees the wall's outer face: its bounce rays leave the scene.)"""
    out = reach("16", pose_files[pose, (152, 150)])
    print(out)
    lines = node_lines(out)
    assert [f["rays"] for f in lines] == ["camera", "bounce"], out
    for f in lines:
        assert f["mismatches"] == "0" and int(f["newRewalks"]) <= int(f["oldRewalks"]), f
    assert int(lines[0]["trusted"]) > 500 and int(lines[0]["hits"]) > 500, lines[0]
    assert (int(lines[1]["hits"]) > 500) == (pose != "partly_behind"), lines[1]


def test_re_walks_of_the_flagship_frame(reach, tmp_path):
    """The Cornell box at 1920x1080, 6 camera rays per tile: the strict test sends the rays that meet the light quad's half in
    the mesh (element 15: its leaf box begins in the triangle's own plane) to the reference's tree; at the found distance only
    those whose entry exceeds t by rounding remain."""
    p = str(tmp_path / "box_1080p.bin")
    pose_blob("box", (1920, 1080)).tofile(p)
    out = reach("6", p)
    print(out)
    cam, bnc = node_lines(out)
    for f in (cam, bnc):
        assert f["mismatches"] == "0" and int(f["trusted"]) > 0, f
    old = int(cam["oldRewalks"]) + int(bnc["oldRewalks"])
    new = int(cam["newRewalks"]) + int(bnc["newRewalks"])
    print(f"re-walks among {int(cam['queries']) + int(bnc['queries'])} queries: {old} with entry < t, {new} with entry <= t")
    assert old > 0 and new < old, out


@pytest.mark.parametrize("pose", POSES)
def test_fma_form_passes_every_box_it_must(slab, pose_files, pose):
    out = slab("boxes", pose_files[pose, (152, 150)])
    print(out)
    (f,) = node_lines(out)
    assert f["omissions"] == "0" and int(f["required"]) > 10000 and int(f["passed"]) >= int(f["required"]) and int(f["leaves"]) == 18, f


@pytest.mark.parametrize("pose", POSES)
def test_no_leaf_the_fma_form_passes_is_missing_from_a_tile_list(slab, pose_files, pose):
    out = slab("rays", pose_files[pose, (152, 150)], pose_files[pose, (61, 45)])
    print(out)
    lines = node_lines(out)
    assert len(lines) == 2, out
    for f in lines:
        assert f["omissions"] == "0" and int(f["required"]) > 0 and int(f["leaves"]) == 18, f

