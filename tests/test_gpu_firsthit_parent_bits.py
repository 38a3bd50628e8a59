"""The read-only passes over the resident scene - guide planes, matte planes, ray queries, the camera rays handed out
(qa_gbuffer.hip, qa_matte.hip, qa_ray_query.hip, qa_radiance.hip) - against the bits they had before their camera ray, hit reset,
material lookup and first-hit colour were folded into qa_firsthit.h: a SHA-256 per output plane, recorded in
tests/golden/firsthit_parent_bits.json with the library built from the commit that file names.  The other tests hold depth, ids and
albedo to the oracle bit for bit, but the normals only to each other (ray queries = guide planes = matte reduced) and to float64
geometry within 1e-4; inside that tolerance all three could move together, and this test would see it.  The kernels are built with
-ffp-contract=off and correctly rounded division and square root: the digests do not depend on the optimiser.

64x48 frames, the region (5, 3) - (52, 43) of gbuffer_util (ragged tiles on both edges, origin off zero); the five scenes of
gbuffer_util.SCENES (all four <RES, TEX> instances) and custom_softshadow.xml, whose camera has a lens: the guide planes and the
sample-0 camera rays take its two draws, the matte planes and the per-sample camera rays refuse such a camera and have no case.

Run this file as a program to record the digests anew (only where a change of the outputs is meant), with QA_HIP_LIB naming the
library to record from:
    QA_HIP_LIB=.../libqaray_hip.so python tests/test_gpu_firsthit_parent_bits.py [commit]"""
import hashlib
import os

import numpy as np
import pytest

import conftest  # noqa: F401  (first: it puts the repository on sys.path when this file runs as a program)
import parent_bits_util as pb
from gbuffer_util import REGION, SCENES, SEEDS, scene_blob

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "firsthit_parent_bits.json")
LENS_SCENE = "custom_softshadow.xml"
ALL_SCENES = list(SCENES) + [LENS_SCENE]
H, W = REGION[3] - REGION[1], REGION[2] - REGION[0]
# sample counts of a frame that stopped early in places: 0 (nothing), 3 (below spp = 5), 9 (above it: the pixel takes 5)
NS_PLANE = np.array([0, 3, 9], np.uint32)[(np.arange(W)[None, :] + 2 * np.arange(H)[:, None]) % 3]
assert NS_PLANE.shape == (H, W) and set(np.unique(NS_PLANE)) == {0, 3, 9}


def label(scene):
    return os.path.basename(scene)


def calls(scene):
    """The calls of one scene, in a fixed order: (name, function of (context, earlier results) -> dict plane -> numpy array)."""
    def cast(seed):
        return lambda c, r: c.cast_rays(*rays(r, seed))

    def rays(r, seed):
        cr = r[f"camera_rays seed={seed}"]
        return cr["origins"], cr["dirs"]

    def occluded(seed, factor):
        return lambda c, r: {"out": c.occluded(*rays(r, seed), np.float32(factor) * r[f"cast_rays seed={seed}"]["t"])}

    def sample_rays(c, r):
        out = c.camera_sample_rays_device(REGION, first=1, count=3)
        c.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}

    out = [(f"gbuffer seed={seed}", lambda c, r, seed=seed: c.gbuffer(REGION, seed)) for seed in SEEDS]
    if scene != LENS_SCENE:
        out += [("matte spp=1", lambda c, r: c.matte(REGION, 1)), ("matte spp=5", lambda c, r: c.matte(REGION, 5)),
                ("matte spp=5 ns=0,3,9", lambda c, r: c.matte(REGION, 5, ns=NS_PLANE))]
    for seed in SEEDS:
        out.append((f"camera_rays seed={seed}", lambda c, r, seed=seed: dict(zip(("origins", "dirs"), c.camera_rays(REGION, seed)))))
    for seed in SEEDS:
        out.append((f"cast_rays seed={seed}", cast(seed)))
        out.append((f"occluded seed={seed} tmax=t/2", occluded(seed, 0.5)))
        out.append((f"occluded seed={seed} tmax=2t", occluded(seed, 2.0)))
    if scene != LENS_SCENE:
        out.append(("camera_sample_rays first=1 count=3", sample_rays))
    return out


def cases():
    return [(scene, name) for scene in ALL_SCENES for name, _ in calls(scene)]


def case_id(scene, name):
    return f"{label(scene)} {name}"


def digest(a):
    a = np.ascontiguousarray(a)
    return f"{a.dtype.name}{list(a.shape)} " + hashlib.sha256(a.tobytes()).hexdigest()


def run_scene(scene):
    """case id -> {plane: digest} of every call of one scene, on one context"""
    from qaray_amd import hip
    blob = scene_blob(scene)
    assert (float(hip.blob_camera(blob)["dof"]) > 0.1) == (scene == LENS_SCENE), scene
    c = hip.Context(0)
    try:
        c.upload_scene(blob)
        results = {}
        for name, fn in calls(scene):
            results[name] = fn(c, results)
        return {case_id(scene, name): {k: digest(v) for k, v in planes.items()} for name, planes in results.items()}
    finally:
        c.close()


def record(commit):
    digests = {}
    for scene in ALL_SCENES:
        digests.update(run_scene(scene))
    return pb.save(GOLDEN, commit, "dtype, shape and SHA-256 of every output plane of the calls in cases() of tests/test_gpu_firsthit_parent_bits.py, "
                   "taken on an MI355X with the library built from that commit", digests)


def test_the_record_names_every_case_and_nothing_else():
    assert pb.names_match(GOLDEN, [case_id(scene, name) for scene, name in cases()])


@pytest.fixture(scope="module")
def computed():
    """scene -> its digests, each scene computed once on first use"""
    cache = {}

    def of(scene):
        if scene not in cache:
            cache[scene] = run_scene(scene)
        return cache[scene]
    return of


@pytest.mark.gpu
@pytest.mark.parametrize("scene,name", cases(), ids=[case_id(s, n) for s, n in cases()])
def test_first_hit_passes_keep_the_parents_bits(computed, scene, name):
    got, want = computed(scene)[case_id(scene, name)], pb.load(GOLDEN)[case_id(scene, name)]
    print(case_id(scene, name), got)
    assert got == want


if __name__ == "__main__":
    pb.main(record, f" from {os.environ.get('QA_HIP_LIB', 'qaray_amd/lib')}")
