"""Parity tests proper: the HIP path (through the C ABI) against the CPU oracle and the reference's
golden vectors, on a real MI355X.

Tolerances (fp32 radiance, written here as the contract asks):
  * sample counts, first-hit depth, ray-cast counters: EXACT (integer / bit-exact).
  * radiance: scenes whose paths have at most one bounce after the camera hit and no lights
    (Cornell box = BASELINE config[1]) are bit-identical to the reference.  Elsewhere the kernel sums
    the reference's recursive radiance formula front-to-back (a throughput product instead of nested
    multiplications), which moves results by a few ulp: per-image RMSE <= 1e-6 and max abs error
    <= 1e-4 (north_star: RMSE < 1e-4).  sinf/cosf/expf/powf/asinf return glibc's bits: their host builds
    against libm in tests/test_device_math.py (with the sphere's double-atan2/asin uv against the oracle's
    expressions), their device builds against the host builds in tests/test_gpu_device_math.py (sin/cos:
    test_device_sincos_equals_host_libm below).  Every shipped kernel instance: tests/test_gpu_variant_census.py.
"""
import os

import numpy as np
import pytest

from conftest import bits, ensure_assets, golden_blob, load_golden, reference_input_names

pytestmark = pytest.mark.gpu

RMSE_TOL = 1e-6
MAXABS_TOL = 1e-4
SUPPORTED = ["c1_sphere_256x256_1spp", "c2_box_64x64_4spp", "c2_box_1080p_crop_8spp", "c2_box_1080p_edge_crop_64spp",
             "c2_box_1080p_crop_512spp", "c3_object_1080p_crop_256spp", "c4_caustics_4k_crop_1024spp", "c5_tower_4k_crop_2048spp",
             "blinn_48x36_4spp", "box3_48x36_4spp", "project4_48x36_4spp", "glass_48x36_8spp", "glossy_48x36_8spp",
             "coffee_48x36_4spp_bounce2", "sphere_adaptive_64x48_4to32spp",
             "textures_80x60_2spp", "softshadow_dof_60x45_2spp",
             "c3_object_1080p_crop_2spp", "c4_caustics_4k_crop_4spp", "c5_tower_4k_crop_2spp"]
BIT_EXACT = ["c2_box_64x64_4spp", "c2_box_1080p_crop_8spp", "c2_box_1080p_edge_crop_64spp", "c2_box_1080p_crop_512spp"]


@pytest.fixture(scope="module")
def ctx():
    from qaray_amd import hip
    c = hip.Context(0)
    yield c
    c.close()


def rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


@pytest.mark.parametrize("name", SUPPORTED)
def test_hip_matches_reference_goldens(ctx, name):
    rgb, depth, ns, meta = load_golden(name)
    ctx.upload_scene(golden_blob(meta))
    ctx.reset_counters()
    g_rgb, g_depth, g_ns = ctx.render_region(tuple(meta["crop"]), meta["spp_min"], max_bounce=meta["bounce"],
                                             seed=meta["seed"], spp_max=meta["spp_max"])
    cnt = ctx.counters()
    assert np.array_equal(g_ns, ns)
    assert np.array_equal(bits(g_depth), bits(depth))
    assert cnt["samples"] == meta["samples"]
    assert cnt["casts_normal"] == meta["casts_normal"] and cnt["casts_shadow"] == meta["casts_shadow"]
    if name in BIT_EXACT:
        assert np.array_equal(bits(g_rgb), bits(rgb))
    else:
        assert rmse(g_rgb, rgb) <= RMSE_TOL
        assert float(np.abs(g_rgb - rgb).max()) <= MAXABS_TOL


@pytest.mark.parametrize("name", reference_input_names())
def test_every_reference_input_hip_vs_oracle(ctx, name):
    """All 28 inputs/*.xml of the reference: none is refused, sample counts, first-hit
    depth and cast counters are exact, radiance within the module's tolerances (scaled by the frame's largest
    value where that exceeds 1).  The oracle is
    pinned to the live reference on the same 28 files by tests/test_oracle_vs_reference.py."""
    from oracle import binding as oracle
    from qaray_amd.host import load_scene_blob
    ensure_assets()
    w, h, spp = 40, 30, 2
    blob = load_scene_blob(name, size=(w, h))
    ctx.upload_scene(blob)
    ctx.reset_counters()
    rgb, depth, ns = ctx.render_region((0, 0, w, h), spp)
    cnt = ctx.counters()
    o_rgb, o_depth, o_ns, o_cnt = oracle.render(blob, (0, 0, w, h), spp)
    assert np.array_equal(ns, o_ns) and np.array_equal(bits(depth), bits(o_depth))
    assert (cnt["samples"], cnt["casts_normal"], cnt["casts_shadow"]) == (o_cnt.samples, o_cnt.casts_normal, o_cnt.casts_shadow)
    assert np.isfinite(rgb).all() == np.isfinite(o_rgb).all()
    scale = max(1.0, float(np.abs(o_rgb[np.isfinite(o_rgb)]).max()) if np.isfinite(o_rgb).any() else 1.0)
    assert float(np.nanmax(np.abs(rgb - o_rgb))) <= MAXABS_TOL * scale
    assert rmse(np.nan_to_num(rgb), np.nan_to_num(o_rgb)) <= RMSE_TOL * scale


def test_hip_matches_oracle_with_traversal_counters(ctx):
    """Same seeded inputs through both implementations, including BVH-node / triangle-test counts."""
    from oracle import binding as oracle
    from qaray_amd.host import load_scene_blob
    blob = load_scene_blob("example_project12_box.xml", size=(160, 90))
    ctx.upload_scene(blob)
    ctx.reset_counters()
    g = ctx.render_region((0, 0, 160, 90), 16, stats=True)
    cnt = ctx.counters()
    o_rgb, o_depth, o_ns, ocnt = oracle.render(blob, (0, 0, 160, 90), 16)
    assert np.array_equal(bits(g[0]), bits(o_rgb)) and np.array_equal(bits(g[1]), bits(o_depth))
    assert (cnt["bvh_nodes"], cnt["tri_tests"]) == (ocnt.bvh_nodes, ocnt.tri_tests)
    assert cnt["pixels"] == 160 * 90


@pytest.mark.parametrize("scene,size,spp", [("example_project12_box.xml", (960, 540), 32), ("custom_textures.xml", (480, 360), 8),
                                            ("custom_photon.xml", (320, 240), 4)])
def test_own_search_tree_equals_reference_tree_walk(ctx, scene, size, spp):
    """LDS-resident scenes: the default kernels search meshes with the library's SAH tree and validate
    the hit against the reference tree's rules (qa_kernel.h hitMesh); the counting kernels walk the
    reference's cy::BVH exactly as the reference does.  Both must return the same bits - here on
    10^7..10^8 casts per scene, far more than the goldens hold."""
    from qaray_amd.host import load_scene_blob
    w, h = size
    ctx.upload_scene(load_scene_blob(scene, size=size))
    ctx.reset_counters()
    a = ctx.render_region((0, 0, w, h), spp)
    ca = ctx.counters()
    ctx.reset_counters()
    b = ctx.render_region((0, 0, w, h), spp, stats=True)
    cb = ctx.counters()
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(a[2], b[2])
    assert (ca["samples"], ca["casts_normal"], ca["casts_shadow"]) == (cb["samples"], cb["casts_normal"], cb["casts_shadow"])
    assert cb["tri_tests"] > 0 and ca["tri_tests"] == 0


def _write_fuzz_scene(tmp, rng, kind):
    """A small OBJ (no .mtl: one XML material) that provokes the cases in which the reference's mesh
    search is not plain geometry: coplanar / duplicated triangles (ties), axis-aligned sheets (flat boxes),
    needles, shared edges, and rays that start on the surface."""
    import os
    v, f = [], []
    def tri(a, b, c):
        base = len(v)
        v.extend([a, b, c])
        f.append((base + 1, base + 2, base + 3))
    if kind == "soup":
        for _ in range(40):
            c = rng.uniform(-4, 4, 3)
            tri(*(c + rng.uniform(-2, 2, (3, 3))))
    elif kind == "sheets":     # grids of axis-aligned quads, each split into two triangles; some sheets doubled
        for z in (-2.0, 0.0, 0.0, 3.0):
            for i in range(3):
                for j in range(3):
                    x0, y0 = -4.5 + 3 * i, -4.5 + 3 * j
                    p = [np.array([x0, y0, z]), np.array([x0 + 3, y0, z]), np.array([x0 + 3, y0 + 3, z]), np.array([x0, y0 + 3, z])]
                    tri(p[0], p[1], p[2])
                    tri(p[0], p[2], p[3])
    elif kind == "needles":
        for _ in range(24):
            c = rng.uniform(-4, 4, 3)
            d = rng.uniform(-1, 1, 3)
            tri(c, c + 6 * d, c + 6 * d + 1e-3 * rng.uniform(-1, 1, 3))
        for _ in range(12):
            c = rng.uniform(-4, 4, 3)
            tri(*(c + rng.uniform(-2, 2, (3, 3))))
    else:                       # "duplicates": random triangles, every third one repeated exactly, some degenerate
        for k in range(30):
            c = rng.uniform(-4, 4, 3)
            t = c + rng.uniform(-2.5, 2.5, (3, 3))
            tri(*t)
            if k % 3 == 0:
                tri(*t)
            if k % 10 == 0:
                tri(t[0], t[0], t[1])
    with open(os.path.join(tmp, "fuzz.obj"), "w") as o:
        for p in v:
            o.write("v %.9g %.9g %.9g\n" % tuple(p))
        for t in f:
            o.write("f %d %d %d\n" % t)
    xml = """<xml><scene>
      <object type="obj" name="fuzz.obj" material="m"><rotate angle="20" x="1" y="0.3" z="0.1"/><translate x="0.5" z="1"/></object>
      <object type="plane" name="floor" material="m"><scale value="30"/><translate z="-6"/></object>
      <material type="blinn" name="m"><diffuse r="0.7" g="0.6" b="0.5"/><specular value="0.3"/><glossiness value="20"/><emission value="0.2"/></material>
      <light type="point" name="l"><intensity value="40"/><position x="3" y="-8" z="9"/></light>
    </scene><camera><position x="0" y="-22" z="6"/><target x="0" y="0" z="0"/><up x="0" y="0" z="1"/><fov value="40"/>
      <width value="128"/><height value="96"/></camera></xml>"""
    path = os.path.join(tmp, "fuzz.xml")
    open(path, "w").write(xml)
    return path


def _write_edge_scene(tmp, n, offset):
    """n x n cells of two isolated axis-aligned right triangles each, modelled `offset` away from the object-space origin
    (the node's transform moves them back in front of the camera).  Out there a hit point is rounded to ~6e-8 * offset,
    so the reference's inside test accepts points that far outside a triangle's edges - and outside the (flat) bounding
    box of the cell's two coplanar triangles, which an own search tree without the slack constants has already pruned."""
    import os
    o = float(offset)
    with open(os.path.join(tmp, "edges.obj"), "w") as f:
        k = 0
        for i in range(n):
            for j in range(n):
                # (every cell at its own height: the reference never enters a box of zero thickness, and a mesh in one
                # plane would be invisible to it)
                x, y, z = o + 2 * i - n, o + 2 * j - n, o + 0.01 * ((7 * i + 3 * j) % 11)
                for (a, b) in ((x, y), (x + 0.7, y + 0.7)):
                    f.write("v %.9g %.9g %.9g\nv %.9g %.9g %.9g\nv %.9g %.9g %.9g\n" % (a, b, z, a + 0.6, b, z, a, b + 0.6, z))
                    f.write("f %d %d %d\n" % (3 * k + 1, 3 * k + 2, 3 * k + 3))
                    k += 1
    xml = """<xml><scene>
      <object type="obj" name="edges.obj" material="m"><translate x="%.9g" y="%.9g" z="%.9g"/></object>
      <material type="blinn" name="m"><diffuse r="0.7" g="0.6" b="0.5"/><emission value="0.3"/></material>
      <light type="point" name="l"><intensity value="60"/><position x="3" y="-8" z="12"/></light>
    </scene><camera><position x="0.3" y="-0.7" z="%.9g"/><target x="0" y="0" z="0"/><up x="0" y="1" z="0"/><fov value="50"/>
      <width value="128"/><height value="96"/></camera></xml>""" % (-o, -o, -o, 2.2 * n)
    path = os.path.join(tmp, "edges.xml")
    open(path, "w").write(xml)
    return path


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("kind", ["soup", "sheets", "needles", "duplicates"])
def test_own_search_tree_fuzz(ctx, tmp_path, kind, seed):
    """Random meshes built to hit the corners of the reference's mesh search (ties, flat boxes, needles,
    degenerate and duplicated triangles): default kernel == counting kernel bit for bit, both == oracle in depth and cast counts."""
    from oracle import binding as oracle
    from qaray_amd.host import load_scene_blob
    rng = np.random.default_rng(10 * seed + {"soup": 1, "sheets": 2, "needles": 3, "duplicates": 4}[kind])
    xml = _write_fuzz_scene(str(tmp_path), rng, kind)
    w, h, spp = 192, 144, 8
    blob = load_scene_blob(xml, size=(w, h), asset_root=str(tmp_path))
    ctx.upload_scene(blob)
    a = ctx.render_region((0, 0, w, h), spp)
    ctx.reset_counters()
    b = ctx.render_region((0, 0, w, h), spp, stats=True)
    cb = ctx.counters()
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))
    o = oracle.render(blob, (0, 0, w, h), spp)
    assert np.array_equal(bits(o[1]), bits(b[1]))
    # (node / triangle counters are not compared here: inside a mesh the reference's shadow query walks on
    # after its first hit, objects.cpp:342-419, while the kernels return at once - same answer, fewer steps)
    assert (cb["casts_normal"], cb["casts_shadow"]) == (o[3].casts_normal, o[3].casts_shadow)
    assert rmse(np.nan_to_num(b[0]), np.nan_to_num(o[0])) <= RMSE_TOL


def test_full_baseline_frame_own_tree_equals_reference_walk(ctx):
    """The whole BASELINE C2 frame at its quoted settings (1920x1080, 512 spp, 1.58e9 casts): the default kernel (own SAH
    tree + the validation rules of hitMesh) and the counting kernel (the reference's cy::BVH walked as the reference walks
    it) return the same bits in every pixel, and the same sample / cast counts."""
    from qaray_amd.host import load_scene_blob
    W, H, spp = 1920, 1080, 512
    ctx.upload_scene(load_scene_blob("example_project12_box.xml", size=(W, H)))
    ctx.reset_counters()
    a = ctx.render_region((0, 0, W, H), spp)
    ca = ctx.counters()
    ctx.reset_counters()
    b = ctx.render_region((0, 0, W, H), spp, stats=True)
    cb = ctx.counters()
    assert ca["samples"] == W * H * spp
    assert (ca["samples"], ca["casts_normal"], ca["casts_shadow"]) == (cb["samples"], cb["casts_normal"], cb["casts_shadow"])
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(a[2], b[2])


_NOSLACK_PROBE = r"""
import sys, tempfile
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
from test_gpu_parity import _write_edge_scene
from qaray_amd.host import load_scene_blob
from qaray_amd import hip
ctx = hip.Context(0)
def differing(blob, w, h, spp, pipeline):
    ctx.set_pipeline(pipeline)
    ctx.upload_scene(blob)
    a = ctx.render_region((0, 0, w, h), spp)
    b = ctx.render_region((0, 0, w, h), spp, stats=True)
    return int((a[0].view(np.uint32) != b[0].view(np.uint32)).any(axis=2).sum() + (a[1].view(np.uint32) != b[1].view(np.uint32)).sum())
tmp = tempfile.mkdtemp()
edge = load_scene_blob(_write_edge_scene(tmp, 28, 4000.0), size=(512, 384), asset_root=tmp)
print("RESULT", differing(load_scene_blob("example_project12_box.xml", size=(1920, 1080)), 1920, 1080, 512, "mega"),
      differing(edge, 512, 384, 16, "mega"), differing(edge, 512, 384, 16, "staged"))
"""


def test_slack_constants_of_the_own_trees_matter():
    """Negative control for the constants that make the own search trees' answers the reference's (box widening by the
    fp32 slack of the reference's inside test, parallelism / cancellation guards: qa_kernel.h hitMesh, qa_widebvh.h).
    `make hip_noslack` builds the library with all of them scaled to zero (QA_SLACK_SCALE=0, test-only).  That build must
    FAIL the checks the product passes: the full C2 frame (own SAH tree vs reference walk: one cast of 1.58e9 goes
    wrong) and a mesh of isolated axis-aligned triangles modelled 4000 units from its origin (4-wide tree, megakernel
    and staged: hits the reference accepts just outside a triangle's box are pruned).  The product library on the same
    inputs: zero differences (second run below; the C2 frame is the test above)."""
    import subprocess
    import sys
    from conftest import ROOT
    lib = os.path.join(ROOT, "qaray_amd", "lib_noslack", "libqaray_hip.so")
    assert os.path.exists(lib), "lib_noslack is missing: __graft_entry__.build() (make hip_noslack) builds it"
    def run(env_extra):
        env = dict(os.environ, **env_extra)
        out = subprocess.run([sys.executable, "-c", _NOSLACK_PROBE, ROOT], env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        return [int(x) for x in [l for l in out.stdout.splitlines() if l.startswith("RESULT")][0].split()[1:]]
    bad = run({"QA_HIP_LIB": lib})
    assert bad[0] > 0, "the C2 frame does not notice the missing slack constants"
    assert bad[1] > 0 and bad[2] > 0, "the far edge mesh does not notice the missing slack constants"
    good = run({"QA_HIP_LIB": ""})
    assert good == [0, 0, 0]


def test_partition_invariance_and_determinism_full_size(ctx):
    """Properties at BASELINE's full frame size (1920x1080): a region rendered alone, as part of a
    bigger region, or as round-robin strips gives the same bits; two runs give the same bits."""
    import torch
    from qaray_amd import distributed as qd, hip
    from qaray_amd.host import load_scene_blob
    W, H, spp = 1920, 1080, 4
    ctx.upload_scene(load_scene_blob("example_project12_box.xml", size=(W, H)))
    full = ctx.render_region((0, 0, W, H), spp)[0]
    again = ctx.render_region((0, 0, W, H), spp)[0]
    assert np.array_equal(bits(full), bits(again))
    crop = ctx.render_region((701, 333, 1222, 801), spp)[0]
    assert np.array_equal(bits(crop), bits(full[333:801, 701:1222]))
    dev = torch.device("cuda", 0)
    world = 3
    parts = []
    for r in range(world):
        n = hip.strip_count(0, H, r, world) * 8
        rgb = torch.zeros((n, W, 3), dtype=torch.float32, device=dev)
        d = torch.zeros((n, W), dtype=torch.float32, device=dev)
        ns = torch.zeros((n, W), dtype=torch.int32, device=dev)
        ctx.render_strips_device((0, 0, W, H), r, world, spp, rgb, d, ns)
        ctx.synchronize()
        parts.append(rgb.cpu().numpy())
    asm = np.zeros((H, W, 3), np.float32)
    for r in range(world):
        qd.place_strips(asm, parts[r], H, world, r)
    assert np.array_equal(bits(asm), bits(full))
    # a different seed changes the image; the first-hit geometry does not depend on the seed
    other = ctx.render_region((0, 0, W, H), spp, seed=12345)
    assert not np.array_equal(bits(other[0]), bits(full))
    # energy sanity: Cornell box radiance is finite and non-negative
    assert np.isfinite(full).all() and (full >= 0).all()


def test_device_blob_upload_equals_host_upload(ctx):
    import torch
    from qaray_amd.host import load_scene_blob
    blob = load_scene_blob("example_project3_sphere.xml", size=(96, 64))
    ctx.upload_scene(blob)
    a = ctx.render_region((0, 0, 96, 64), 2)[0]
    ctx.upload_scene_device(torch.from_numpy(blob).cuda())
    b = ctx.render_region((0, 0, 96, 64), 2)[0]
    assert np.array_equal(bits(a), bits(b))


def test_stop_flag_skips_pixels_and_error_codes(ctx):
    from qaray_amd import hip
    from qaray_amd.host import load_scene_blob
    fresh = hip.Context(0)
    with pytest.raises(hip.HipError) as e:
        fresh.render_region((0, 0, 8, 8), 1)
    assert e.value.code == -5  # QA_ENOSCENE
    blob = load_scene_blob("example_project12_box.xml", size=(64, 64))
    fresh.upload_scene(blob)
    with pytest.raises(hip.HipError) as e:
        fresh.render_region((0, 0, 65, 64), 1)
    assert e.value.code == -1
    with pytest.raises(hip.HipError) as e:
        fresh.upload_scene(blob[:100])
    assert e.value.code == -1
    fresh.upload_scene(blob)
    fresh.request_stop()               # tasking::signal_stop before the render: nothing is rendered
    rgb, depth, ns = fresh.render_region((0, 0, 64, 64), 4)
    assert (ns == 0).all()
    fresh.clear_stop()
    rgb, depth, ns = fresh.render_region((0, 0, 64, 64), 4)
    assert (ns == 4).all()
    # what the HIP path cannot reproduce is refused loudly, never silently approximated:
    # area lights log one record per hit and hold at most 8 (maxBounce <= 7)
    fresh.upload_scene(load_scene_blob("custom_softshadow.xml"))
    with pytest.raises(hip.HipError) as e:
        fresh.render_region((0, 0, 8, 8), 1, max_bounce=9)
    assert e.value.code == -6  # QA_EUNSUPPORTED
    fresh.close()


def test_cli_driver_matches_python_path(tmp_path):
    """qaray_hip (C++ Renderer + the reference's command line) writes the same colorBuffer.png as the
    ctypes path through FrameBuffer."""
    import os
    import subprocess
    from conftest import ROOT
    from qaray_amd import hip
    from qaray_amd.host import FrameBuffer, load_scene_blob, SCENES_DIR
    exe = os.path.join(ROOT, "qaray_amd", "lib", "qaray_hip")
    out = str(tmp_path) + "/"
    r = subprocess.run([exe, "-batch", "-spp", "4", "-size", "96", "64", "-root", SCENES_DIR, "-out", out,
                        os.path.join(SCENES_DIR, "example_project12_box.xml")], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert "Elapsed Time is" in r.stdout
    c = hip.Context(0)
    c.upload_scene(load_scene_blob("example_project12_box.xml", size=(96, 64)))
    rgb, depth, ns = c.render_region((0, 0, 96, 64), 4)
    fb = FrameBuffer(96, 64)
    fb.deposit(0, 0, 96, 64, rgb, depth, ns, 4, use_srgb=True)
    ref = str(tmp_path / "py.png")
    fb.save_image(ref)
    assert open(out + "colorBuffer.png", "rb").read() == open(ref, "rb").read()
    c.close()


def _eightbit_names():
    import os
    from conftest import GOLDEN
    d = os.path.join(GOLDEN, "eightbit")
    return sorted(f[:-4] for f in os.listdir(d) if f.endswith(".npz"))


@pytest.mark.parametrize("name", _eightbit_names())
def test_cli_pngs_equal_the_references_8bit_products(tmp_path, name):
    """the three PNGs the batch driver writes (colorBuffer / depthBuffer / sampleBuffer, as
    Renderer_MPI::Render does) against 8-bit arrays made by the REFERENCE's own code from its own frame
    (tests/golden/eightbit/, oracle/_ref/ref_harness --eight-bit).  Depth and sample-count images: byte for byte
    (their inputs are exact).  Colour: byte for byte on the Cornell box (bit-identical radiance); elsewhere the
    radiance differs from the reference's by a few ulp, which may move a value across a rounding boundary: at most
    one level on at most 0.2 % of the bytes."""
    import json
    import os
    import subprocess
    from PIL import Image
    from conftest import GOLDEN, ROOT
    from qaray_amd.host import SCENES_DIR
    z = np.load(os.path.join(GOLDEN, "eightbit", name + ".npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    exe = os.path.join(ROOT, "qaray_amd", "lib", "qaray_hip")
    out = str(tmp_path) + "/"
    r = subprocess.run([exe, "-batch", "-sppMin", str(meta["spp_min"]), "-sppMax", str(meta["spp_max"]), "-srgb", str(meta["srgb"]),
                        "-seed", str(meta["seed"]), "-size", str(meta["width"]), str(meta["height"]), "-root", SCENES_DIR, "-out", out,
                        os.path.join(SCENES_DIR, meta["scene"])], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    color = np.asarray(Image.open(out + "colorBuffer.png").convert("RGB"))
    zimg = np.asarray(Image.open(out + "depthBuffer.png").convert("L"))
    cimg = np.asarray(Image.open(out + "sampleBuffer.png").convert("L"))
    assert np.array_equal(zimg, z["zimg"])
    assert np.array_equal(cimg, z["countimg"])
    if "box" in name:
        assert np.array_equal(color, z["color"])
    else:
        d = np.abs(color.astype(np.int16) - z["color"].astype(np.int16))
        assert d.max() <= 1 and (d != 0).mean() <= 0.002, (int(d.max()), float((d != 0).mean()))


def test_device_sincos_equals_host_libm(ctx):
    """The device sinf/cosf restate glibc's algorithm; on [0, 2*pi] they return glibc's bits."""
    from qaray_amd import hip
    import ctypes as C
    x = np.concatenate([np.linspace(0, 2 * np.pi, 200001, dtype=np.float32),
                        np.random.default_rng(1).random(300000, dtype=np.float32) * np.float32(6.2831855)])
    s = np.zeros_like(x)
    c = np.zeros_like(x)
    L = hip.lib()
    L.qa_test_sincosf_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    assert L.qa_test_sincosf_device(x.ctypes.data, x.size, s.ctypes.data, c.ctypes.data) == 0
    libm = C.CDLL("libm.so.6")
    libm.sinf.restype = C.c_float
    libm.sinf.argtypes = [C.c_float]
    libm.cosf.restype = C.c_float
    libm.cosf.argtypes = [C.c_float]
    idx = np.random.default_rng(2).choice(x.size, 20000, replace=False)
    hs = np.array([libm.sinf(float(v)) for v in x[idx]], np.float32)
    hc = np.array([libm.cosf(float(v)) for v in x[idx]], np.float32)
    assert np.array_equal(bits(s[idx]), bits(hs)) and np.array_equal(bits(c[idx]), bits(hc))


def test_two_rank_bench_rehearsal_equals_single_rank():
    """bench.py's N>1 path (blob broadcast, round-robin strips, gather, assemble) with two ranks that
    share this box's GPU (gloo transport; the nccl path differs only in where the collectives run)."""
    import json
    import os
    import socket
    import subprocess
    import sys
    from conftest import ROOT
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--check",
           "--steps", "1", "--warmup", "0", "--spp", "4", "--width", "320", "--height", "180", "--cpu-spp", "0"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    assert d["n_gpus"] == 2 and d["check"] is True
    assert d["config"]["frame"] == [453, 255]   # 320x180 scaled by sqrt(2): weak scaling in resolution


@pytest.mark.parametrize("ranks,config,size", [(4, "c4", (384, 216)), (2, "c5", (480, 270))])
def test_strong_scaling_rehearsal_of_baseline_multi_gpu_configs(ranks, config, size):
    """BASELINE C4 / C5 are FIXED frames cut over 4 / 8 GPUs (strong scaling).  Rehearsal of bench.py --config on this
    one-GPU box: the ranks share the GPU, collectives over gloo; the frame must keep its size and the gathered image
    must equal the frame rendered by one rank, bit for bit (the staged integrator and the megakernel both render strips)."""
    import json
    import os
    import socket
    import subprocess
    import sys
    from conftest import ROOT
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", str(ranks), "--backend", "gloo", "--check", "--config", config,
           "--steps", "1", "--warmup", "0", "--spp", "4", "--width", str(size[0]), "--height", str(size[1]), "--cpu-spp", "0", "--pipeline", "staged"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["n_gpus"] == ranks and d["check"] is True and d["scaling"] == "strong"
    assert d["config"]["frame"] == list(size) and d["config"]["baseline_config"] == config



def test_rccl_path_with_one_rank_broadcast_gather_and_all_three_images(tmp_path):
    """The RCCL ("nccl") branch of bench.py on the one GPU there is: torch.distributed.run --nproc-per-node 1 with the process
    group FORCED (init_process_group(device_id), uint8 blob broadcast, dist.gather of the flat colour | depth | sample-count
    buffer on the step's stream, assembly), --check (gathered arrays == the frame rendered alone, bit for bit: all three
    arrays the reference gathers, Renderer_MPI.cpp:194-207) and the three PNGs written from the GATHERED arrays."""
    import json
    import os
    import socket
    import subprocess
    import sys
    from conftest import ROOT
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    prefix = str(tmp_path / "g_")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "1", "--backend", "nccl", "--force-collectives", "--check",
           "--steps", "2", "--warmup", "1", "--spp", "4", "--width", "320", "--height", "180", "--cpu-spp", "0", "--save-png", prefix]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["n_gpus"] == 1 and d["check"] is True
    assert d["collectives"]["backend"] == "nccl" and d["collectives"]["world"] == 1
    for name in ("colorBuffer.png", "depthBuffer.png", "sampleBuffer.png"):
        assert os.path.getsize(prefix + name) > 100, name


@pytest.mark.parametrize("scene,size,spp", [("example_project7_object.xml", (1920, 1080), 8),
                                            ("example_project12_caustics_glossy.xml", (3840, 2160), 4),
                                            ("trc_scene_tower.xml", (3840, 2160), 4)])
def test_cooperative_kernel_equals_the_reference_walk_at_the_quoted_frame_sizes(scene, size, spp):
    """qa_integrate_cs against the counting kernel (the reference's cy::BVH walked as the reference walks it) on the WHOLE
    1080p / 4K frames the BASELINE numbers are quoted on (10^8 casts each): every pixel's radiance, depth and sample count
    bit for bit, cast counters equal."""
    from conftest import bits, ensure_assets
    from qaray_amd import hip
    from qaray_amd.host import load_scene_blob
    ensure_assets()
    w, h = size
    c = hip.Context(0)
    c.upload_scene(load_scene_blob(scene, size=size))
    assert "qa_integrate_cs" in c.kernel_name()
    c.reset_counters()
    a = c.render_region((0, 0, w, h), spp)
    ca = c.counters()
    c.reset_counters()
    b = c.render_region((0, 0, w, h), spp, stats=True)
    cb = c.counters()
    c.close()
    for x, y in zip(a, b):
        assert np.array_equal(bits(x), bits(y))
    assert all(ca[k] == cb[k] for k in ("samples", "casts_normal", "casts_shadow", "pixels"))


@pytest.mark.parametrize("scene,size,spp", [("example_project12_box.xml", (200, 131), 4), ("trc_scene_tower.xml", (160, 90), 2)])
def test_cli_multi_device_path_equals_the_single_context_path(tmp_path, scene, size, spp):
    """qaray_hip -devices 1 takes the C++ multi-GPU route (one host thread + context per device, flattened scene copied
    device-to-device, strips rendered with qa_render_strips_device, peer copy of the packed colour | depth | sample-count
    buffer to the first device, PlaceStrips) - with the one GPU of this box.  Its three PNGs must equal the classic
    single-context CLI's byte for byte (131 rows: a ragged last strip)."""
    import os
    import subprocess
    from conftest import ensure_assets
    from qaray_amd.host import SCENES_DIR
    ensure_assets()
    from conftest import ROOT
    exe = os.path.join(ROOT, "qaray_amd", "lib", "qaray_hip")
    outs = {}
    for mode, extra in (("single", []), ("multi", ["-devices", "1"])):
        out = str(tmp_path / mode) + "_"
        r = subprocess.run([exe, "-batch", "-spp", str(spp), "-size", str(size[0]), str(size[1]), "-root", SCENES_DIR, "-out", out] + extra +
                           [os.path.join(SCENES_DIR, scene)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
        if mode == "multi":
            assert "Running on 1 HIP device(s)" in r.stdout
        outs[mode] = {n: open(out + n, "rb").read() for n in ("colorBuffer.png", "depthBuffer.png", "sampleBuffer.png")}
        outs[mode]["samples"] = [l for l in r.stdout.splitlines() if l.startswith("samples ")][0].split("  ")[0:2]
    assert outs["single"] == outs["multi"]


@pytest.mark.parametrize("case", ["box", "sphere_lights", "textures", "object", "tower", "caustics", "softshadow", "area_coop", "object_staged", "glass_photon"])
def test_frames_do_not_depend_on_stale_scratch(case):
    """The photon-walk nondeterminism of rounds 1 / 2 was hipcc storing a spill ahead of the instruction that re-enables masked
    lanes: the lanes that never stored reloaded whatever the scratch slot held.  Whatever the cause, such a read
    shows when the private segments of every wave slot are filled with different patterns before a frame: here every kernel
    family (LDS-resident with / without lights and textures, cooperative textured / untextured, area lights, staged stages,
    photon gather) renders the same bits after 0, all-ones and 1.0f - the pattern for which the broken kernel happened to be
    right."""
    from qaray_amd import hip
    from qaray_amd.host import load_scene_blob
    ensure_assets()
    scene, size, spp = {"box": ("example_project12_box.xml", (320, 180), 8), "sphere_lights": ("example_project3_sphere.xml", (256, 256), 4),
                        "textures": ("custom_textures.xml", (240, 180), 4), "object": ("example_project7_object.xml", (320, 180), 4),
                        "tower": ("trc_scene_tower.xml", (320, 180), 4), "caustics": ("example_project12_caustics_glossy.xml", (320, 180), 4),
                        "softshadow": ("custom_softshadow.xml", (160, 120), 2), "area_coop": ("example_project10_test.xml", (160, 120), 2), "object_staged": ("example_project7_object.xml", (240, 136), 2),
                        "glass_photon": ("trc_mtl_glass.xml", (96, 72), 2)}[case]
    c = hip.Context(0)
    c.upload_scene(load_scene_blob(scene, size=size))
    if case == "object_staged":
        c.set_pipeline("staged")
    if case == "glass_photon":
        c.build_photon_maps((2000, 20, 2.0), (300, 20, 3.0))
    frames = []
    for pattern in (0x00000000, 0xFFFFFFFF, 0x3F800000):
        c.scrub_scratch(pattern)
        frames.append(c.render_region((0, 0) + size, spp))
    name = c.kernel_name()
    c.close()
    for f in frames[1:]:
        for a, b in zip(f, frames[0]):
            assert np.array_equal(bits(a), bits(b)), name
