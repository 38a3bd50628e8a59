"""Texture edits, the parts that need no GPU: the texel conversion of qa_texel_dev.h compiled for the host (qa_test_texels_host)
against numpy's float32 division and against the texture probes; the patched blobs the GPU tests use as expectations against the
oracle; and the host-only rebuild of the scene side after a texture edit (qa_scene_build.h RebuildSceneSide) under the sanitizers."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, ensure_assets
from test_device_math import same_bits
from test_texture_host import cases, host_probe, probe_blob, queries, tables  # noqa: F401 (probe_blob: fixture)

import texture_edit_util as T

F32 = np.float32


def all_bytes_image(w):
    """Rows of w texels that hold all 256 byte values in every channel, inside rows 3 * w + 5 bytes long -> the (h, w, 3) view."""
    h = -(-256 // w)
    store = np.full((h, 3 * w + 5), 0xA5, np.uint8)
    img = store[:, :3 * w].reshape(h, w, 3)
    v = np.resize(np.arange(256, dtype=np.uint8), h * w)
    img[..., 0], img[..., 1], img[..., 2] = v.reshape(h, w), v[::-1].reshape(h, w), np.roll(v, 85).reshape(h, w)
    assert all(len(np.unique(img[..., c])) == 256 for c in range(3)) and img.strides[0] > 3 * w
    return img


@pytest.mark.parametrize("w", [1, 3, 4, 5, 67])
def test_texels_host_equals_float32_division(w):
    from qaray_amd import hip
    img = all_bytes_image(w)
    got = hip.texels_host(img)
    want = img.astype(F32) / F32(255)
    assert want.dtype == F32
    assert np.array_equal(got[..., :3].view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got[..., 3].view(np.uint32), np.zeros(img.shape[:2], np.uint32))


def test_texels_host_equals_the_texture_probe_at_texel_centres(probe_blob):
    """What an upload tabulates (BuildTextures, through the same header) and what the hook returns for the blob's own texels."""
    from qaray_amd import hip
    tex, _, _ = tables(probe_blob)
    blob = np.array(probe_blob, np.uint8, copy=True)
    checked = 0
    for ti in T.file_textures(blob):
        px = hip.blob_texels(blob, ti)
        h, w = px.shape[:2]
        y, x = np.mgrid[0:h, 0:w]
        x, y = x.ravel(), y.ravel()
        # textureSample reads texel (ix, iy) alone where width * u and height * (1 - v) are the integers themselves (fx = fy = 0)
        u, v = x.astype(F32) / F32(w), F32(1) - y.astype(F32) / F32(h)
        exact = (F32(w) * u == x) & (F32(h) * (F32(1) - v) == y)
        if (w, h) == (8, 8):
            assert exact.all()
        uv = np.stack([u, v, np.zeros(w * h, F32)], axis=1)[exact]
        probe = host_probe(blob, 1, ti, queries(a=uv))[:, :3]
        got = hip.texels_host(px)[..., :3].reshape(-1, 3)[exact]
        assert np.array_equal(probe.view(np.uint32), got.view(np.uint32)), (ti, w, h)
        checked += int(exact.sum())
    assert checked > 50


def scene_blobs():
    from qaray_amd.host import load_scene_blob
    ensure_assets()
    return [load_scene_blob("custom_textures.xml", size=(80, 60)), load_scene_blob("example_project7_object.xml", size=(80, 56))]


def test_patched_blobs_are_pinned_to_the_oracle(probe_blob):
    """Blob B = A with a texel rectangle, a texmap transform, a texmap's texture index, a checker colour and the backdrop colours
    patched: the host build of the texture path on B equals the oracle's on B, on test_texture_host.py's query sets."""
    from oracle import binding as oracle
    b, steps = T.make_b(probe_blob)
    kinds = [s[0] for s in steps]
    assert kinds.count("texmaps") == 2 and {"texels_host", "texels_device", "textures", "backdrop"} <= set(kinds)
    assert not np.array_equal(b, probe_blob)
    total = 0
    for op, index, q in cases(b):
        if op in (0, 6, 7, 8):
            continue   # (no texture table read: test_texture_host.py has them)
        hq = host_probe(b, op, index, q)
        assert same_bits(hq, oracle.texture_probe(b, op, index, q)), (op, index)
        total += len(q)
    assert total > 100000
    changed = sum(not same_bits(host_probe(b, op, index, q), host_probe(probe_blob, op, index, q)) for op, index, q in cases(b) if op in (1, 3, 5))
    assert changed >= 4, "the patches changed no lookup"


def test_rebuild_scene_side_after_texture_edits_under_asan_ubsan(tmp_path, probe_blob):
    """tests/cpp/texture_edit_check.cpp, a program of its own: RebuildSceneSide after every texture patch == BuildScene of the
    patched blob, with and without DropMeshSide; refused records change nothing."""
    from qaray_amd import hip as hipmod
    from test_sanitizers import ENV, SAN
    hipmod.Context.edit_texels   # (the feature, not only the driver, must be there: AttributeError without it)
    hip = os.path.join(ROOT, "qaray_amd", "csrc", "hip")
    exe = str(tmp_path / "texture_edit_check")
    subprocess.run(["g++", "-std=c++17", *SAN, "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{ROOT}/include",
                    f"-I{hip}", os.path.join(ROOT, "tests", "cpp", "texture_edit_check.cpp"), os.path.join(hip, "qa_scene_build.cpp"), "-o", exe],
                   check=True)
    files = []
    for k, blob in enumerate([probe_blob] + scene_blobs()):
        p = str(tmp_path / f"scene{k}.bin")
        np.asarray(blob, np.uint8).tofile(p)
        files.append(p)
    r = subprocess.run([exe, *files], env=ENV, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "texture_edit_check: clean" in r.stdout, r.stdout[-3000:]
    assert "runtime error" not in r.stdout and "AddressSanitizer" not in r.stdout, r.stdout[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ".bin: " in ln]
    assert len(lines) == len(files), r.stdout[-3000:]
    for ln in lines:
        for step in ("texel rectangle", "texmap transform", "texmap rebound", "checker colours", "backdrop colours", "refused: texture type",
                     "refused: texture width", "refused: texel offset", "refused: texture index = count", "refused: background texmap",
                     "after the refusals"):
            assert step in ln, ln
