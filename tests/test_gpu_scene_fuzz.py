"""Scene-content fuzz, GPU leg: the generated scenes of tests/scene_fuzz_util.py (materials, lights, transforms, cameras,
contacts; tests/test_scene_fuzz_host.py pins the oracle to the reference on the same files) through the HIP kernels on a real
MI355X, against the CPU oracle's frame of the same flat scene.

Every case: the upload is not refused; the per-lane megakernel (option "coop" = 0) returns the oracle's sample counts, first-hit
depth bits and samples / casts_normal / casts_shadow, is non-finite in exactly the oracle's elements, and over the finite ones
stays within test_gpu_parity.py's radiance tolerances (imported, scaled by the frame's largest value where that exceeds 1, as
there); the oracle's frame is the one the manifest records of the reference (hashes), so the chain HIP -> oracle -> reference
closes on this machine too.  Siblings bit for bit, counters included, each named by kernel_name(): the counting variant (the
reference's tree, walked as the reference walks it), for every scene in global memory what option "coop" = 1 runs it on (for
the `big` cases, a mesh beyond LDS, that must be the cooperative kernel) and, where a `big` scene is staged-eligible, the staged
integrator.  Two cases per family are also rendered as two regions cut at a row
that is no multiple of the 8-row tile, and must give the whole frame's bits and counters."""
import numpy as np
import pytest

import scene_fuzz_util as fz
from conftest import bits
from test_gpu_parity import MAXABS_TOL, RMSE_TOL

pytestmark = pytest.mark.gpu

LIVE = fz.live_cases()
COUNTERS = ("samples", "casts_normal", "casts_shadow")
# two cases per family rendered in two regions: odd frames (37x52, 52x37), one of each pair adaptive; lights: area lights
# with adaptive sampling, and nine lights
REGION_SEEDS = {f: (1, 2) for f in fz.FAMILIES}
REGION_SEEDS["lights"] = (5, 9)
REGION_CASES = [(f, s) for f, n in fz.FAMILIES.items() for s in REGION_SEEDS[f] if (f, s) in LIVE]


@pytest.fixture(scope="module")
def ctx():
    from qaray_amd import hip
    c = hip.Context(0)
    yield c
    c.set_pipeline("auto")
    c.set_option("coop", 1)
    c.close()


def _frame(ctx, o, region=None, stats=False):
    """-> (rgb, depth, ns), counters of one frame of the case's settings, and the name of the kernel it ran on."""
    p = o["params"]
    ctx.reset_counters()
    out = ctx.render_region(region or (0, 0, p["width"], p["height"]), p["spp_min"], max_bounce=p["bounce"], spp_max=p["spp_max"],
                            stats=stats)
    return out, ctx.counters(), ctx.kernel_name()


def _upload(ctx, o, coop, pipeline="mega"):
    ctx.set_option("coop", coop)
    ctx.set_pipeline(pipeline)
    ctx.upload_scene(o["blob"])     # (a refusal raises HipError: a finding, not a skip)


def _same(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def _lights(blob):
    """-> (shadow-casting lights, any of them with a size) of a flat scene."""
    from qaray_amd.hip import blob_table
    t = blob_table(np.array(blob), "lights")
    shadow = t[t["type"] != 0]      # QA_LIGHT_AMBIENT = 0
    return len(shadow), bool((shadow["size"] > 0).any())


@pytest.mark.parametrize("case", LIVE, ids=fz.case_id)
def test_kernels_equal_the_oracle_and_their_siblings(ctx, case):
    family, seed = case
    big = family == "big"
    e, o = fz.manifest()[case], fz.oracle_frame(*case)
    # the oracle's frame is the recorded reference's
    assert fz.sha(o["rgb"].tobytes()) == e["rgb_sha256"] and fz.sha(o["depth"].tobytes()) == e["depth_sha256"]
    o_cnt = (o["cnt"].samples, o["cnt"].casts_normal, o["cnt"].casts_shadow)

    # the per-lane megakernel against the oracle
    _upload(ctx, o, coop=0)
    (rgb, depth, ns), cnt, name = _frame(ctx, o)
    # (the small scenes are LDS-resident or not by their node count; the height field never is)
    assert name.startswith("qa_integrate<RES=0," if big else "qa_integrate<RES=") and "counting" not in name, name
    assert np.array_equal(ns, o["ns"])
    assert np.array_equal(bits(depth), bits(o["depth"]))
    assert tuple(cnt[k] for k in COUNTERS) == o_cnt
    finite = np.isfinite(o["rgb"])
    assert np.array_equal(np.isfinite(rgb), finite)
    if finite.any():
        scale = max(1.0, float(np.abs(o["rgb"][finite]).max()))
        d = rgb[finite].astype(np.float64) - o["rgb"][finite].astype(np.float64)
        maxabs, err = float(np.abs(d).max()), float(np.sqrt(np.mean(d ** 2)))
        print(f"scene fuzz {fz.case_id(case)} | {name} | scale {scale:.3g} max abs {maxabs:.3g} rmse {err:.3g}")
        assert maxabs <= MAXABS_TOL * scale
        assert err <= RMSE_TOL * scale

    # siblings, bit for bit
    sib, sib_cnt, sib_name = _frame(ctx, o, stats=True)
    assert "counting variant" in sib_name, sib_name
    assert _same(sib, (rgb, depth, ns)) and all(sib_cnt[k] == cnt[k] for k in COUNTERS), sib_name
    if "RES=0" in name:
        # every scene in global memory, the small ones with many nodes included: what option "coop" = 1 picks for it
        _upload(ctx, o, coop=1)
        sib, sib_cnt, sib_name = _frame(ctx, o)
        assert not big or sib_name.startswith("qa_integrate_cs<"), sib_name
        print(f"scene fuzz {fz.case_id(case)} | coop=1: {sib_name}")
        assert _same(sib, (rgb, depth, ns)) and all(sib_cnt[k] == cnt[k] for k in COUNTERS), sib_name
    if not big:
        return
    # staged-eligible as tests/test_gpu_staged.py decides it: the context says so once the pipeline is asked for.  The staged
    # integrator takes at most 4 shadow-casting lights and no area lights; the rest of these scenes is within its limits
    _upload(ctx, o, coop=0, pipeline="staged")
    n_shadow, area = _lights(o["blob"])
    assert ("staged" in ctx.kernel_name()) == (n_shadow <= 4 and not area), ctx.kernel_name()
    if "staged" in ctx.kernel_name():
        sib, sib_cnt, sib_name = _frame(ctx, o)
        assert sib_name.startswith("staged"), sib_name
        st = ctx.staged_stats()
        assert st["jobs_done"] == st["jobs_queued"] > 0
        assert _same(sib, (rgb, depth, ns)) and all(sib_cnt[k] == cnt[k] for k in COUNTERS), sib_name


@pytest.mark.parametrize("case", REGION_CASES, ids=fz.case_id)
def test_two_regions_equal_the_whole_frame(ctx, case):
    """The frame cut at a row inside a tile (and, for the second seed, at a column inside a tile): every pixel owns its
    random-number stream and its Halton index, so both parts return the whole frame's bits and their counters add up to its."""
    o = fz.oracle_frame(*case)
    w, h = o["params"]["width"], o["params"]["height"]
    _upload(ctx, o, coop=1 if case[0] == "big" else 0)
    whole, cnt, _ = _frame(ctx, o)
    if case[1] == REGION_SEEDS[case[0]][0]:
        cut = h // 2 + 3
        parts = [(0, 0, w, cut), (0, cut, w, h)]
        join = lambda a, b: np.concatenate([a, b], axis=0)
    else:
        cut = w // 2 + 3
        parts = [(0, 0, cut, h), (cut, 0, w, h)]
        join = lambda a, b: np.concatenate([a, b], axis=1)
    assert cut % 8 != 0
    (a, ca, _), (b, cb, _) = (_frame(ctx, o, region=r) for r in parts)
    assert _same([join(x, y) for x, y in zip(a, b)], whole)
    assert all(ca[k] + cb[k] == cnt[k] for k in COUNTERS)
