"""Bake maps on the CPU: the host build of qaray_amd/csrc/hip/qa_bake_dev.h (hip.bake_texels_host, hip.bake_dilate_host: the source the
kernels of qa_bake.hip are compiled from) against the float32 numpy restatement of the header's opening comment in tests/bake_util.py,
bit for bit; the `face` plane against the inside rule in rational arithmetic (exactly on a dyadic atlas, watertight on a generic chart);
point and normal against a float64 restatement within a tolerance derived from the operands; tiles, texmaps, the material filter, the
plane, the refusals; the gutter fill; tests/cpp/bake_check.cpp runs the same functions stand-alone under AddressSanitizer + UBSan."""
import os
import subprocess

import numpy as np
import pytest

import bake_util as B
from conftest import ROOT
from qaray_amd import hip

F32 = np.float32


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    return B.build_cases(tmp_path_factory.mktemp("bake"))


@pytest.fixture(scope="module")
def maps(cases):
    """Every case at every size through the host build, made once: (name, (W, H)) -> planes"""
    return {(name, size): hip.bake_texels_host(c["blob"], c["node"], *size, texmap=c["texmap"], mtl=c["mtl"]) for name, c in cases.items() for size in c["sizes"]}


def same_bits(x, y):
    return all(np.array_equal(x[k].view(np.uint32), y[k].view(np.uint32)) for k in hip.BAKE_PLANES)


def test_host_build_equals_the_restatement_bit_for_bit(cases, maps):
    for (name, size), got in maps.items():
        c = cases[name]
        ref = B.bake_ref(c["blob"], c["node"], *size, c["texmap"], c["mtl"])
        assert same_bits(got, ref), (name, size)
        unc = got["face"] < 0
        assert not got["point"][unc].any() and not got["normal"][unc].any() and not got["bary"][unc].any(), (name, size)
    # a subset of the planes gives the same bits as all four
    c = cases["chart"]
    one = hip.bake_texels_host(c["blob"], c["node"], 19, 13, planes=("bary",))
    assert list(one) == ["bary"] and np.array_equal(B.bits(one["bary"]), B.bits(maps[("chart", (19, 13))]["bary"]))


def test_dyadic_atlas_is_exact(cases, maps):
    """uv on multiples of 1/64, W and H powers of two: every operation of the inside rule is exact, so the plane equals the rational
    rule everywhere - shared edges, vertices, the diagonal through samples, the lowest face under the overlap, the void faces"""
    c = cases["atlas"]
    faces = B.mesh_arrays(c["blob"], 0)["faces"]
    assert len(faces) == 7 and (faces[6]["vt"] == -1).all()
    for size in c["sizes"]:
        got = maps[("atlas", size)]["face"]
        exact, _ = B.exact_faces(c["blob"], c["node"], *size)
        print(f"atlas {size}: {(got >= 0).sum()} covered texels")
        assert np.array_equal(got, exact), size
        assert set(np.unique(got)) == {-1, 0, 1, 2, 3, 4}          # faces 5 (zero area) and 6 (no vt) never win
        # samples on the shared diagonal of chart A belong to the lower face, the overlap goes to the charts
        assert (got >= 0).sum() > 500


def test_generic_chart_is_watertight(cases, maps):
    """The jittered chart over the whole texture, and the convex case's chart inset from the texture's border (there samples do lie
    outside every face, so the second assertion can fail)"""
    for name, sizes in (("chart", ((19, 13), (64, 64))), ("convex", ((19, 13), (48, 40)))):
        c = cases[name]
        for size in sizes:
            W, H = size
            got = maps[(name, size)]["face"]
            exact, margin = B.exact_faces(c["blob"], c["node"], W, H)
            if name == "chart":
                sx, sy = B.samples(W, H)
                inner = ((sx > 1e-6) & (sx < 1 - 1e-6))[None, :] & ((sy > 1e-6) & (sy < 1 - 1e-6))[:, None]
                assert (got[inner] >= 0).all(), "a crack: a sample inside the chart's rectangle that no face holds"
            else:
                assert (exact < 0).sum() > 20 and (got[exact >= 0] >= 0).all(), "a crack"
            assert not ((got >= 0) & (exact < 0)).any(), "a texel is covered whose sample lies outside every face"
            differ = (got != exact) & (got >= 0)
            near = int(((margin <= 1e-6) & (got >= 0)).sum())
            print(f"{name} {size}: {int(differ.sum())} of {int((got >= 0).sum())} covered texels differ from the exact lowest face; {near} lie within 1e-6 of an edge")
            assert (margin[differ] <= 1e-6).all()
            assert differ.sum() <= 0.01 * (got >= 0).sum()


def test_point_and_normal_against_float64(cases, maps):
    for name in ("nested", "grid264", "plane", "texmap"):
        c = cases[name]
        size = c["sizes"][0]
        got = maps[(name, size)]
        cov = got["face"] >= 0
        P, N, scale = B.point_normal_f64(c["blob"], c["node"], got["face"], got["bary"])
        levels = B.chain_levels(c["blob"], c["node"])
        tol_p = B.point_tolerance(scale, levels)
        tol_n = B.normal_tolerance(levels, B.chain_stretch(c["blob"], c["node"]))
        err_p = np.abs(got["point"].astype(np.float64) - P).max(axis=2)
        err_n = np.abs(got["normal"].astype(np.float64) - N).max(axis=2)
        print(f"{name}: {levels} levels; point error / tolerance at most {(err_p[cov] / tol_p[cov]).max():.3f}; normal error {err_n[cov].max():.2e} of {tol_n:.2e}")
        assert cov.any() and (err_p[cov] <= tol_p[cov]).all() and (err_n[cov] <= tol_n).all(), name
        assert np.abs(np.linalg.norm(got["normal"][cov].astype(np.float64), axis=1) - 1).max() < 4e-7
    assert B.chain_levels(cases["nested"]["blob"], 2) == 2


def test_uv_of_the_weights_is_the_sample(cases, maps):
    """T0 a + T1 b + T2 c, in float64 from the stored (a, b), is S + (m, n) for integers m, n, to the tolerance of the point test:
    B.point_tolerance with the texture vertices in the vertices' place and no node above them (levels = 0: the 7 roundings of the
    interpolation, of the largest term a weight times a texture vertex gives)."""
    for name in ("chart", "tile_up", "tile_negative", "straddle", "texmap", "convex"):
        c = cases[name]
        size = c["sizes"][0]
        W, H = size
        got = maps[(name, size)]
        sx, sy = B.samples(W, H)
        T = {f: B.texture_vertices(c["blob"], uv, c["texmap"]).astype(np.float64) for f, uv, _, _ in B.node_faces(c["blob"], c["node"]) if uv is not None}
        worst = 0.0
        for iy, ix in zip(*np.nonzero(got["face"] >= 0)):
            t = T[int(got["face"][iy, ix])]
            a, b = (float(v) for v in got["bary"][iy, ix])
            w = np.array([a, b, 1 - a - b])
            off = w @ t - np.array([sx[ix], sy[iy]], np.float64)
            tol = B.point_tolerance(np.abs(w[:, None] * t).max(), 0)
            worst = max(worst, np.abs(off - np.round(off)).max() / tol)
            assert np.abs(off - np.round(off)).max() <= tol, (name, ix, iy)
        print(f"{name}: uv error / tolerance at most {worst:.3f}")


def test_tiles_texmaps_and_the_material_filter(cases, maps, tmp_path):
    up, neg, straddle = (maps[(n, (19, 13))]["face"] for n in ("tile_up", "tile_negative", "straddle"))
    # a chart of half a tile's side covers about a quarter of the texels wherever it is placed; one two tiles wide wraps around
    assert 40 <= (up >= 0).sum() <= 90 and 40 <= (neg >= 0).sum() <= 90 and (straddle >= 0).sum() > 150
    t = cases["texmap"]
    rec = hip.blob_table(t["blob"], "texmaps")[t["texmap"]]
    assert rec["texture"] >= 0 and abs(rec["itm"][0]) < 1e-6 and abs(rec["itm"][1]) > 0.4       # scaled and turned by 90 degrees
    raw = hip.bake_texels_host(t["blob"], t["node"], 32, 16)
    assert not np.array_equal(raw["face"], maps[("texmap", (32, 16))]["face"])
    both, red, blue = (maps[(f"two_mtl_{m}", (19, 13))]["face"] for m in (-1, 0, 1))
    faces = B.mesh_arrays(cases["two_mtl_0"]["blob"], 0)["faces"]
    assert sorted(np.unique(faces["mtl"])) == [0, 1]
    assert (faces["mtl"][red[red >= 0]] == 0).all() and (faces["mtl"][blue[blue >= 0]] == 1).all()
    assert np.array_equal(np.where(red >= 0, red, blue), both)   # (samples on an edge between the two lie in both: the lower face)
    none = hip.bake_texels_host(cases["two_mtl_0"]["blob"], 1, 19, 13, mtl=7)
    assert (none["face"] == -1).all()
    plane = maps[("plane", (16, 16))]
    assert set(np.unique(plane["face"])) == {0, 1}


def refused(code, *args, **kw):
    with pytest.raises(hip.HipError) as e:
        hip.bake_texels_host(*args, **kw)
    assert e.value.code == code, e.value
    return str(e.value)


def test_refusals(cases, tmp_path):
    c = cases["chart"]
    blob = c["blob"]
    for w, h in ((0, 4), (4, 0), (8193, 4), (4, 8193)):
        refused(B.EINVAL, blob, 1, w, h)
    L = hip.lib()
    assert L.qa_test_bake_texels_host(blob.ctypes.data, blob.size, 1, -1, -1, 4, 4, None, None, None, None) == B.EINVAL   # no plane
    refused(B.EINVAL, blob, 0, 4, 4)          # the root: a node without an object
    refused(B.EINVAL, blob, 2, 4, 4)          # out of range
    refused(B.EINVAL, blob, -1, 4, 4)
    refused(B.EINVAL, blob, 1, 4, 4, texmap=0)   # the scene has no texmap
    # a face over five tiles: refused, the outputs untouched
    five = B.write_scene(tmp_path / "five", B.mesh_node("s.obj"), {"s.obj": B.span_obj(5)})
    assert B.over_tiles(five, 1)
    face = np.full((4, 4), 77, np.int32)
    point = np.full((4, 4, 3), 5.0, F32)
    rc = L.qa_test_bake_texels_host(five.ctypes.data, five.size, 1, -1, -1, 4, 4, point.ctypes.data, None, face.ctypes.data, None)
    assert rc == B.EUNSUPPORTED and (face == 77).all() and (point == 5.0).all()
    four = B.write_scene(tmp_path / "four", B.mesh_node("s.obj"), {"s.obj": B.span_obj(4)})
    assert not B.over_tiles(four, 1) and (hip.bake_texels_host(four, 1, 8, 8)["face"] >= 0).any()
    # a sphere, a mesh without texture vertices, a texmap without a texture
    sphere = B.write_scene(tmp_path / "sphere", '<object type="sphere" name="s" material="m"/>')
    assert "sphere" in refused(B.EUNSUPPORTED, sphere, 1, 4, 4)
    bare = B.write_scene(tmp_path / "bare", B.mesh_node("b.obj"), {"b.obj": "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n"})
    refused(B.EINVAL, bare, 1, 4, 4)
    t = cases["texmap"]
    edited = t["blob"].copy()
    hip.blob_table(edited, "texmaps")["texture"][t["texmap"]] = -1
    refused(B.EINVAL, edited, t["node"], 4, 4, texmap=t["texmap"])
    refused(B.EINVAL, t["blob"], t["node"], 4, 4, texmap=len(hip.blob_table(t["blob"], "texmaps")))
    # not a blob at all
    assert L.qa_test_bake_texels_host(blob.ctypes.data, 64, 1, -1, -1, 4, 4, None, None, face.ctypes.data, None) == B.EINVAL
    with pytest.raises(ValueError):
        hip.bake_texels_host(blob, 1, 4, 4, planes=("depth",))


# ---- the gutter fill

def picture(h, w, seed=1):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def test_dilation_equals_the_restatement():
    rng = np.random.default_rng(11)
    for (h, w), density in (((13, 19), 0.3), ((16, 16), 0.05), ((5, 3), 0.2), ((1, 1), 0.0), ((40, 33), 0.01)):
        rgb = picture(h, w, h)
        face = np.where(rng.random((h, w)) < density, 3, -1).astype(np.int32)
        for radius in (0, 1, 2, 8):
            assert np.array_equal(hip.bake_dilate_host(rgb, face, radius), B.dilate_ref(rgb, face, radius)), (h, w, radius)


def test_dilation_rules():
    rgb = picture(5, 5)
    face = np.full((5, 5), -1, np.int32)
    # radius 0 is the identity, whatever is covered
    face[1, 3] = 0
    assert np.array_equal(hip.bake_dilate_host(rgb, face, 0), rgb)
    # the tie order: four covered texels at distance 1 of the centre -> the one above (dy = -1); two at dy = 0 -> the left one
    face[:] = -1
    for y, x in ((1, 2), (3, 2), (2, 1), (2, 3)):
        face[y, x] = 0
    out = hip.bake_dilate_host(rgb, face, 1)
    assert (out[2, 2] == rgb[1, 2]).all()
    face[1, 2] = face[3, 2] = -1
    assert (hip.bake_dilate_host(rgb, face, 1)[2, 2] == rgb[2, 1]).all()
    # covered texels keep their bytes; the nearer wins over the earlier
    face[:] = -1
    face[0, 0], face[2, 3] = 0, 0
    out = hip.bake_dilate_host(rgb, face, 2)
    assert (out[0, 0] == rgb[0, 0]).all() and (out[2, 2] == rgb[2, 3]).all() and (out[1, 1] == rgb[0, 0]).all()
    # wrap across both borders: the only covered texel is the last one, the first one reaches it at (-1, -1)
    face[:] = -1
    face[4, 4] = 0
    out = hip.bake_dilate_host(rgb, face, 1)
    assert (out[0, 0] == rgb[4, 4]).all() and (out[0, 4] == rgb[4, 4]).all() and (out[4, 0] == rgb[4, 4]).all()
    # nothing in reach: its own bytes
    assert (out[2, 2] == rgb[2, 2]).all()
    assert np.array_equal(out, B.dilate_ref(rgb, face, 1))


def test_dilation_refusals():
    rgb, face = picture(4, 4), np.zeros((4, 4), np.int32)
    with pytest.raises(hip.HipError) as e:
        hip.bake_dilate_host(rgb, face, 2, out=rgb)
    assert e.value.code == B.EINVAL
    with pytest.raises(hip.HipError):
        hip.bake_dilate_host(rgb, face, 9)
    with pytest.raises(ValueError):
        hip.bake_dilate_host(rgb, face.astype(np.int64), 1)
    with pytest.raises(ValueError):
        hip.bake_dilate_host(rgb, np.zeros((4, 5), np.int32), 1)
    L = hip.lib()
    assert L.qa_test_bake_dilate_host(rgb.ctypes.data, None, 4, 4, 1, rgb.ctypes.data) == B.EINVAL
    out = np.zeros_like(rgb)
    assert L.qa_test_bake_dilate_host(rgb.ctypes.data, face.ctypes.data, 0, 4, 1, out.ctypes.data) == B.EINVAL


def test_constants():
    assert hip.BAKE_PLANES == ("point", "normal", "face", "bary")
    assert (hip.QA_BAKE_MAX_DIM, hip.QA_BAKE_MAX_RADIUS, hip.QA_BAKE_MAX_TILES) == (8192, 8, 4)
    header = open(os.path.join(ROOT, "qaray_amd", "csrc", "hip", "qa_bake_dev.h")).read()
    for text in ("#define QA_BAKE_MAX_TILES 4", "#define QA_BAKE_MAX_DIM 8192u", "#define QA_BAKE_MAX_RADIUS 8u"):
        assert text in header


def test_header_functions_under_asan_ubsan(tmp_path):
    """tests/cpp/bake_check.cpp: the header's host half on heap buffers of exactly their size, stand-alone under ASan / UBSan (nothing
    is loaded into Python under a sanitizer)."""
    from test_sanitizers import ENV, SAN
    exe = str(tmp_path / "bake_check")
    subprocess.run(["g++", "-std=c++17", *SAN, "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{ROOT}/include",
                    f"-I{ROOT}/qaray_amd/csrc/hip", os.path.join(ROOT, "tests", "cpp", "bake_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], env=ENV, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "bake_check: clean" in r.stdout, r.stdout[-3000:]
    assert "runtime error" not in r.stdout and "AddressSanitizer" not in r.stdout, r.stdout[-3000:]
