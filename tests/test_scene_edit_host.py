"""Scene edits, the parts that need no GPU: HostScene.set_camera / camera(), the host-only rebuild of the scene-side tables
(qa_scene_build.h RebuildSceneSide) under the sanitizers, and the oracle's view of an edited blob."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, bits, ensure_assets

import scene_edit_util as U

CAMERA_SCENES = [("example_project12_box.xml", (64, 64)), ("custom_softshadow.xml", (48, 36)), ("example_project7_object.xml", (40, 28))]


@pytest.mark.parametrize("name,size", CAMERA_SCENES)
def test_set_camera_equals_loading_the_rewritten_xml(tmp_path, name, size):
    from qaray_amd import host
    ensure_assets()
    cam = U.moved_camera(U.xml_camera(U.scene_path(name)))
    dst = str(tmp_path / name)
    U.write_xml_with_camera(U.scene_path(name), dst, cam, size)
    want = host.HostScene(dst, asset_root=host.SCENES_DIR).flatten()
    s = host.HostScene(U.scene_path(name), size=size)
    before = s.flatten()
    s.set_camera(cam["pos"], cam["target"], cam["up"], cam["fov"], cam["focaldist"], cam["dof"])
    got = s.flatten()
    assert not np.array_equal(before, got), "the camera did not move"
    assert np.array_equal(got, want)
    # the block alone, without a flatten: the header's bytes 16..92
    assert s.camera().tobytes() == want[16:92].tobytes()
    # None keeps fov / focaldist / dof
    s.set_camera(cam["pos"], cam["target"], cam["up"])
    assert np.array_equal(s.flatten(), want)
    assert s.size == size


def test_rebuild_scene_side_equals_a_fresh_build_under_asan_ubsan(tmp_path):
    """RebuildSceneSide after patching the camera, a light, a material, a depth-1 and a depth-2 node (and the plan-changing
    light and root edits) == BuildScene of the patched blob: every vector, DScene and ScenePlan (tests/cpp/scene_edit_check.cpp)."""
    from qaray_amd.host import load_scene_blob
    from qaray_amd import hip as hipmod
    from test_sanitizers import ENV, SAN
    from test_gpu_progressive import FAMILIES
    hipmod.Context.edit_camera   # (the feature, not only the driver, must be there: AttributeError without it)
    hip = os.path.join(ROOT, "qaray_amd", "csrc", "hip")
    exe = str(tmp_path / "scene_edit_check")
    subprocess.run(["g++", "-std=c++17", *SAN, "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{ROOT}/include",
                    f"-I{hip}", os.path.join(ROOT, "tests", "cpp", "scene_edit_check.cpp"), os.path.join(hip, "qa_scene_build.cpp"), "-o", exe],
                   check=True)
    ensure_assets()
    scenes = sorted({(scene, size) for scene, size, _, _ in FAMILIES.values()})
    files = []
    for scene, size in scenes:
        p = str(tmp_path / f"{scene}.bin")
        load_scene_blob(scene, size=size).tofile(p)
        files.append(p)
    r = subprocess.run([exe, *files], env=ENV, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "scene_edit_check: clean" in r.stdout, r.stdout[-3000:]
    assert "runtime error" not in r.stdout and "AddressSanitizer" not in r.stdout, r.stdout[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ".bin: " in ln]
    assert len(lines) == len(files), r.stdout[-3000:]
    for ln in lines:
        for step in ("camera", "material colours", "depth-1 node", "root node moved"):
            assert step in ln, ln
        assert "light moved and dimmed" in ln or "no lights" in ln, ln   # (the Cornell box is lit by an emitter)
    # nodes inside a group exist in some of the families (the tower, the textured objects)
    assert any("depth-2 node" in ln for ln in lines), r.stdout[-3000:]
    assert sum("light moved and dimmed" in ln for ln in lines) >= len(lines) - 1
    assert any("light size across 0.01" in ln for ln in lines) and any("light made ambient" in ln for ln in lines)


@pytest.mark.parametrize("name,size", CAMERA_SCENES[:2])
def test_oracle_sees_the_edited_camera(tmp_path, name, size):
    """The blob a context hands back after edit_camera is blob A with B's camera block: the oracle's frame of it differs from A's
    (the edit is not a no-op) and equals the frame of the XML-rewritten blob bit for bit."""
    from oracle import binding as oracle
    from qaray_amd import hip
    ensure_assets()
    a = U.host_scene(name, size)
    blob_a = a.flatten()
    cam = U.moved_camera(U.xml_camera(U.scene_path(name)))
    a.set_camera(cam["pos"], cam["target"], cam["up"], cam["fov"], cam["focaldist"], cam["dof"])
    edited = blob_a.copy()
    hip.blob_camera(edited)[...] = a.camera()
    dst = str(tmp_path / name)
    U.write_xml_with_camera(U.scene_path(name), dst, cam, size)
    from qaray_amd import host
    blob_b = host.HostScene(dst, asset_root=host.SCENES_DIR).flatten()
    region = (0, 0) + size
    fa = oracle.render(blob_a, region, 4)[:3]
    fe = oracle.render(edited, region, 4)[:3]
    fb = oracle.render(blob_b, region, 4)[:3]
    assert not np.array_equal(bits(fa[0]), bits(fe[0])), "the edited camera renders the same frame"
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(fe, fb))
