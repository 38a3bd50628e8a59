"""Scene-content fuzz, CPU leg: the generated scenes of tests/scene_fuzz_util.py (materials, lights, transforms, cameras,
contacts; one family each, with that family's edge values in every seed) through this repo's loader and the oracle, against
what the REAL reference made of the same files: recorded (tests/golden/scene_fuzz/manifest.json: hashes and counters, by
tests/golden/make_goldens.py scene_fuzz) and, where oracle/_ref/ref_harness is built, live.  Bit for bit: radiance, first-hit
depth, sample counts and the three counters.  fz.oracle_frame() keeps one oracle frame per case; the GPU leg
(tests/test_gpu_scene_fuzz.py) compares the kernels with it."""
import json
import os
import subprocess

import numpy as np
import pytest

import scene_fuzz_util as fz
from conftest import bits
from oracle import binding as oracle
from qaray_amd.seed import DEFAULT_SEED

LIVE = fz.live_cases()


def test_manifest_covers_every_case_and_respects_the_drop_cap():
    m = fz.manifest()
    assert sorted(m) == sorted(fz.cases())
    for family, n in fz.FAMILIES.items():
        dropped = [s for s in range(n) if "dropped" in m[(family, s)]]
        assert n >= 4 and len(dropped) <= 1 and n - len(dropped) >= 3, (family, dropped)


@pytest.mark.parametrize("case", fz.cases(), ids=fz.case_id)
def test_generator_is_deterministic(case):
    """The generated text equals what the manifest's results were recorded on (dropped cases included), and so do the frames."""
    e = fz.manifest()[case]
    d, xml = fz.scene_dir(*case)
    assert sorted(e["files"]) == sorted([os.path.basename(xml)] + fz.asset_names(case[0]))
    for name, digest in e["files"].items():
        with open(os.path.join(d, name), "rb") as f:
            assert fz.sha(f.read()) == digest, name
    assert {k: e[k] for k in ("width", "height", "spp_min", "spp_max", "bounce")} == fz.params(*case)


@pytest.mark.parametrize("case", LIVE, ids=fz.case_id)
def test_oracle_equals_recorded_reference_bit_for_bit(case):
    e, o = fz.manifest()[case], fz.oracle_frame(*case)
    assert fz.sha(o["ns"].tobytes()) == e["ns_sha256"]
    assert fz.sha(o["depth"].tobytes()) == e["depth_sha256"]
    assert fz.sha(o["rgb"].tobytes()) == e["rgb_sha256"]
    assert (o["cnt"].samples, o["cnt"].casts_normal, o["cnt"].casts_shadow) == (e["samples"], e["casts_normal"], e["casts_shadow"])
    assert int((~np.isfinite(o["rgb"]).all(axis=2)).sum()) == e["nonfinite_rgb_pixels"]


def _harness(case, *extra):
    d, xml = fz.scene_dir(*case)
    p = fz.params(*case)
    out = os.path.join(d, "ref")
    cmd = [oracle.REF_HARNESS, os.path.basename(xml), "--size", str(p["width"]), str(p["height"]), "--spp-min", str(p["spp_min"]),
           "--spp-max", str(p["spp_max"]), "--bounce", str(p["bounce"]), "--seed", str(DEFAULT_SEED), "--threads", "4", "--out", out, *extra]
    r = subprocess.run(cmd, cwd=d, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-300:]
    return out, p


needs_harness = pytest.mark.skipif(not os.path.exists(oracle.REF_HARNESS),
                                   reason="oracle/_ref/ref_harness is only built where the reference's sources are")


@needs_harness
@pytest.mark.parametrize("case", LIVE, ids=fz.case_id)
def test_oracle_equals_live_reference_bit_for_bit(case):
    out, p = _harness(case)
    o = fz.oracle_frame(*case)
    h, w = p["height"], p["width"]
    with open(out + ".json") as f:
        meta = json.load(f)
    assert np.array_equal(np.fromfile(out + ".ns.u32", np.uint32).reshape(h, w), o["ns"])
    assert np.array_equal(bits(np.fromfile(out + ".depth.f32", np.float32).reshape(h, w)), bits(o["depth"]))
    ref = np.fromfile(out + ".rgb.f32", np.float32).reshape(h, w, 3)
    assert np.array_equal(np.isfinite(ref), np.isfinite(o["rgb"]))
    assert np.array_equal(bits(ref), bits(o["rgb"]))
    assert (o["cnt"].samples, o["cnt"].casts_normal, o["cnt"].casts_shadow) == (meta["samples"], meta["casts_normal"], meta["casts_shadow"])


@needs_harness
@pytest.mark.parametrize("case", [c for c in LIVE if c[0] in ("transforms", "lights")], ids=fz.case_id)
def test_loader_equals_the_references_scene_dump(case):
    """Node matrices and their inverses (mirrors, 1e3 axis ratios, cancelling translations, depth 8), the camera frame, the
    shared cube's arrays and search tree, the light count: what the reference's loader built, bit for bit."""
    from test_host_layer import assert_blob_equals_dump, parse_blob
    d, _ = fz.scene_dir(*case)
    dump = os.path.join(d, "dump.json")
    _harness(case, "--dump-scene", dump, "--no-render")
    with open(dump) as f:
        assert_blob_equals_dump(parse_blob(fz.oracle_frame(*case)["blob"]), json.load(f))


def _shadow_lights(blob):
    from qaray_amd.hip import blob_table
    return int((blob_table(np.array(blob), "lights")["type"] != 0).sum())   # QA_LIGHT_AMBIENT = 0


@pytest.mark.parametrize("case", LIVE, ids=fz.case_id)
def test_every_case_exercises_its_family(case):
    """From the oracle's frame alone: a family must not pass while its rays miss everything."""
    family, seed = case
    o = fz.oracle_frame(*case)
    p, cnt = o["params"], o["cnt"]
    assert (o["depth"] < 1e30).mean() >= 0.25
    base = fz.BIG_OF[seed][0] if family == "big" else family
    if base in ("dielectric", "lobes", "camera") and p["bounce"] > 0:
        assert cnt.casts_normal > cnt.samples          # (camera: the frames 1 wide and 1 high see a reflecting sphere too)
    if base == "lights":
        assert (cnt.casts_shadow > 0) == (_shadow_lights(o["blob"]) > 0)


def test_families_cover_the_listed_light_counts_and_indices():
    from qaray_amd.hip import blob_table
    counts = {_shadow_lights(fz.oracle_frame(*c)["blob"]) for c in LIVE if c[0] == "lights"}
    assert {0, 1, 4, 5, 6, 9} <= counts
    iors = set()
    for c in LIVE:
        if c[0] == "dielectric":
            got = {float(v) for v in blob_table(np.array(fz.oracle_frame(*c)["blob"]), "materials")["ior"]}
            assert {float(np.float32(i)) for i in fz.INDICES} <= got, c    # every seed carries every index
            iors |= got
    assert {float(np.float32(i)) for i in fz.INDICES} <= iors
    bounces = {fz.params(*c)["bounce"] for c in LIVE if c[0] == "dielectric"}
    assert bounces >= {1, 5, 7} and len([c for c in LIVE if c[0] == "dielectric"]) >= 3
    depths = {int(blob_table(np.array(fz.oracle_frame(*c)["blob"]), "instances")["depth"].max()) for c in LIVE if c[0] == "transforms"}
    assert 8 in depths and depths <= set(fz.DEPTHS)
