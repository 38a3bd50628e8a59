"""The host forms of the queries, one after another on one context (qaray_amd/csrc/hip/qa_stage.h carves the one staging buffer they
share): the same buffer reused, regrown and reused under another layout.  Every host form's output is compared, bit for bit, with
the device form of the same call on the same inputs - the reference; with the host form asked for each output alone; and, for a form
with an optional input, with the device form without it.  The library's C entries are called directly: the Python wrappers of the host
forms always ask for every plane.  One scene (the teapot of the ray-query tests, 64 x 48), shapes of a few dozen elements."""
import ctypes as C

import numpy as np
import pytest

from gbuffer_util import SEEDS, scene_blob
from ray_query_util import TEAPOT

pytestmark = pytest.mark.gpu
SEED = SEEDS[0]
F32, I32, U32, U8 = np.float32, np.int32, np.uint32, np.uint8


class Case:
    """One call: the entry's name without "qa_" (its device form is name + "_device"), the inputs name -> array (`optional`: the ones
    that may be left out), the outputs name -> (dtype, shape) (`required`: the ones the entry refuses to go without), and args(p): the
    argument list behind the context from p, name -> pointer or None"""

    def __init__(self, name, ins, outs, args, optional=(), required=()):
        self.name, self.ins, self.outs, self.args, self.optional, self.required = name, ins, outs, args, optional, required


def region_case(kind, region, rng):
    x0, y0, x1, y1 = region
    h, w = y1 - y0, x1 - x0
    ns = rng.integers(0, 5, (h, w)).astype(U32)
    if kind == "gbuffer":
        return Case("gbuffer_region", {}, {"normal": (F32, (h, w, 3)), "albedo": (F32, (h, w, 3)), "depth": (F32, (h, w)), "ids": (I32, (h, w, 2))},
                    lambda p: [x0, y0, x1, y1, SEED, p["normal"], p["albedo"], p["depth"], p["ids"]])
    if kind == "matte":
        return Case("matte_region", {"ns": ns}, {"coverage": (F32, (h, w)), "albedo": (F32, (h, w, 3)), "normal": (F32, (h, w, 3)), "backdrop": (F32, (h, w, 3))},
                    lambda p: [x0, y0, x1, y1, 3, p["ns"], p["coverage"], p["albedo"], p["normal"], p["backdrop"]], optional=("ns",))
    if kind == "idmatte":
        return Case("idmatte_region", {"ns": ns}, {"ids": (I32, (h, w, 8)), "counts": (U32, (h, w, 8)), "other": (U32, (h, w)), "samples": (U32, (h, w))},
                    lambda p: [x0, y0, x1, y1, 3, p["ns"], 0, p["ids"], p["counts"], p["other"], p["samples"]], optional=("ns",))
    assert kind == "ao"
    return Case("ao_region", {"ns": ns}, {"open": (U32, (h, w)), "rays": (U32, (h, w)), "ao": (F32, (h, w))},
                lambda p: [x0, y0, x1, y1, 1, 3, p["ns"], 4, 2.5, SEED, p["open"], p["rays"], p["ao"]], optional=("ns",))


def ray_case(kind, rays, n, rng, per_sample=False):
    """rays: origins, dirs, and the points and normals they hit (zeros where they hit nothing: void points), of at least n records"""
    from qaray_amd import hip
    o, d, pts, nrm = (np.ascontiguousarray(a[:n]) for a in rays)
    sid = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(U32)
    if kind == "cast":
        return Case("cast_rays", {"o": o, "d": d}, {"t": (F32, (n,)), "ids": (I32, (n, 2)), "normal": (F32, (n, 3)), "point": (F32, (n, 3))},
                    lambda p: [n, p["o"], p["d"], p["t"], p["ids"], p["normal"], p["point"]])
    if kind == "occluded":
        tmax = rng.uniform(0, 80, n).astype(F32)
        return Case("occluded", {"o": o, "d": d, "tmax": tmax}, {"out": (U8, (n,))}, lambda p: [n, p["o"], p["d"], p["tmax"], p["out"]], required=("out",))
    if kind == "ao_points":
        return Case("ao_points", {"points": pts, "normals": nrm, "stream_ids": sid.view(I32)}, {"open": (U32, (n,)), "ao": (F32, (n,))},
                    lambda p: [n, p["points"], p["normals"], p["stream_ids"], 2, 5, 2.5, SEED, p["open"], p["ao"]], optional=("stream_ids",))
    if kind == "irradiance":
        par = hip.RadianceParams.of(2, 1, SEED)
        return Case("irradiance_points", {"points": pts, "normals": nrm, "stream": sid}, {"rgb": (F32, (n, 3)), "ns": (U32, (n,))},
                    lambda p: [n, p["points"], p["normals"], p["stream"], C.byref(par), p["rgb"], p["ns"]], optional=("stream",), required=("rgb",))
    assert kind == "radiance"
    spp = 3 if per_sample else 2
    par = hip.RadianceParams.of(spp, 1, SEED, per_sample=per_sample)
    if per_sample:   # a record per ray and sample: the ray's own, nudged
        o = np.repeat(o[:, None], spp, axis=1)
        d = np.ascontiguousarray(d[:, None] + rng.uniform(-0.01, 0.01, (n, spp, 3)).astype(F32))
    rec = d.shape[:-1]
    dx, dy = (np.ascontiguousarray(d + rng.uniform(-0.002, 0.002, d.shape).astype(F32)) for _ in range(2))
    screen = rng.uniform(0, 48, rec + (2,)).astype(F32)
    return Case("radiance_rays", {"o": o, "d": d, "dx": dx, "dy": dy, "screen": screen, "stream": sid}, {"rgb": (F32, (n, 3)), "t": (F32, (n,)), "ns": (U32, (n,))},
                lambda p: [n, p["o"], p["d"], p["dx"], p["dy"], p["screen"], p["stream"], C.byref(par), p["rgb"], p["t"], p["ns"]],
                optional=("dx+dy", "screen", "stream"), required=("rgb",))


def probe_case(vis, rng):
    from qaray_amd import hip
    n, m, d = 2, 2, 1
    points = np.array([[0.2, -3.0, 1.0], [-1.5, -1.0, 2.5]], F32)
    sid = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(U32)
    par, vp = hip.ProbeParams.of(m, 1, 1, SEED), hip.ProbeVisParams.of(d, 6.0)
    outs = {"sh": (F32, (n, 9, 3)), "cube": (F32, (n, 6, m, m, 3)), "hits": (U32, (n,)), "tmin": (F32, (n,))}
    if not vis:
        return Case("probe_sh", {"points": points, "stream": sid}, outs,
                    lambda p: [n, p["points"], p["stream"], C.byref(par), p["sh"], p["cube"], p["hits"], p["tmin"]], optional=("stream",), required=("sh",))
    outs["moments"] = (F32, (n, 6, d, d, 2))
    return Case("probevis_sh", {"points": points, "stream": sid}, outs,
                lambda p: [n, p["points"], p["stream"], C.byref(par), C.byref(vp), p["sh"], p["cube"], p["hits"], p["tmin"], p["moments"]],
                optional=("stream",), required=("moments",))


def bake_case():
    w, h = 5, 3
    return Case("bake_texels", {}, {"point": (F32, (h, w, 3)), "normal": (F32, (h, w, 3)), "face": (I32, (h, w)), "bary": (F32, (h, w, 2))},
                lambda p: [2, -1, -1, w, h, p["point"], p["normal"], p["face"], p["bary"]])   # node 2: the pot, a mesh with texture vertices


def fresh_output(spec):
    """A plane of 0xCD bytes: what the call does not write stays recognisable, and is the same on both sides"""
    dtype, shape = spec
    return np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, 0xCD, U8).view(dtype).reshape(shape)


def given(case, without):
    return {k: v for k, v in case.ins.items() if k not in without.split("+")}


def call(ctx, case, want=None, without="", device=False):
    """The host form, or the device form on the context's stream -> name -> array of the outputs asked for (`want`: all)"""
    import torch
    from qaray_amd import hip
    ins, outs = given(case, without), {k: fresh_output(case.outs[k]) for k in (want or case.outs)}
    if device:
        dev = torch.device("cuda", 0)
        t_in, t_out = ({k: torch.from_numpy(v.reshape(-1).view(U8)).to(dev) for k, v in group.items()} for group in (ins, outs))
        torch.cuda.synchronize(dev)
        p = {k: {**t_in, **t_out}[k].data_ptr() if (k in t_in or k in t_out) else None for k in list(case.ins) + list(case.outs)}
        rc = getattr(hip.lib(), f"qa_{case.name}_device")(ctx._h, *case.args(p), None)
    else:
        p = {k: {**ins, **outs}[k].ctypes.data if (k in ins or k in outs) else None for k in list(case.ins) + list(case.outs)}
        rc = getattr(hip.lib(), f"qa_{case.name}")(ctx._h, *case.args(p))
    assert rc == 0, (case.name, want, without, device, rc, hip.lib().qa_last_error().decode())
    if device:
        ctx.synchronize()
        outs = {k: t_out[k].cpu().numpy().view(case.outs[k][0]).reshape(case.outs[k][1]) for k in outs}
    return outs


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.reshape(-1).view(U8), b.reshape(-1).view(U8))


@pytest.fixture(scope="module")
def bench():
    """The context, and the cases in the order they are called: rays of 65 and of 1, regions of 9 x 7 and 8 x 8, 5 x 3 texels, 2
    probes; a form comes back under another shape only after forms of other layouts have had the buffer"""
    from ray_query_util import fresh
    ctx = fresh(scene_blob(TEAPOT))
    try:
        rng = np.random.default_rng(20)
        o, d = ctx.camera_rays((20, 16, 33, 21), SEED)   # 13 x 5 = 65 rays at the pot and the ground around it
        d[[3, 40, 64]] *= -1                             # (and three into the sky: their hit points are void points)
        hit = ctx.cast_rays(o, d)
        assert 0 < (hit["t"] < 1e29).sum() < len(o)
        rays = (o, d, hit["point"], hit["normal"])
        odd, even = (5, 3, 14, 10), (8, 8, 16, 16)
        cases = [ray_case("cast", rays, 65, rng), region_case("gbuffer", odd, rng), ray_case("occluded", rays, 65, rng), region_case("matte", even, rng),
                 ray_case("cast", rays, 1, rng), region_case("idmatte", odd, rng), bake_case(), region_case("ao", even, rng),
                 ray_case("ao_points", rays, 65, rng), ray_case("radiance", rays, 65, rng), probe_case(False, rng), ray_case("irradiance", rays, 1, rng),
                 probe_case(True, rng), ray_case("radiance", rays, 1, rng, per_sample=True), region_case("gbuffer", even, rng),
                 ray_case("irradiance", rays, 65, rng), region_case("matte", odd, rng), region_case("idmatte", even, rng), region_case("ao", odd, rng),
                 ray_case("ao_points", rays, 1, rng), ray_case("occluded", rays, 1, rng), ray_case("cast", rays, 65, rng)]
        yield ctx, cases, [call(ctx, case, device=True) for case in cases]
    finally:
        ctx.close()


def test_all_twelve_host_forms_are_in_the_sequence(bench):
    assert {case.name for case in bench[1]} == {"gbuffer_region", "matte_region", "idmatte_region", "ao_region", "ao_points", "cast_rays", "occluded",
                                                "bake_texels", "radiance_rays", "irradiance_points", "probe_sh", "probevis_sh"}


def test_host_forms_in_sequence_are_the_device_forms(bench):
    ctx, cases, reference = bench
    for i, (case, want) in enumerate(zip(cases, reference)):
        got = call(ctx, case)
        for k in case.outs:
            assert same_bits(got[k], want[k]), (i, case.name, k)
            assert (got[k].reshape(-1).view(U8) != 0xCD).any(), (i, case.name, k, "not written")


def test_each_output_alone_is_the_output_among_all(bench):
    ctx, cases, reference = bench
    for i, (case, all_outputs) in enumerate(zip(cases, reference)):
        alone = [tuple(case.required)] if case.required and len(case.outs) > len(case.required) else []
        alone += [tuple(case.required) + (k,) for k in case.outs if k not in case.required]
        for want in alone:
            got = call(ctx, case, want=want)
            for k in want:
                assert same_bits(got[k], all_outputs[k]), (i, case.name, want, k)


def test_without_an_optional_input_is_the_device_form_without_it(bench):
    ctx, cases, reference = bench
    for i, case in enumerate(cases):
        for without in case.optional:
            got, want = call(ctx, case, without=without), call(ctx, case, without=without, device=True)
            for k in case.outs:
                assert same_bits(got[k], want[k]), (i, case.name, without, k)
        if case.name == "radiance_rays" and case.outs["rgb"][1][0] == 65:   # (the ids reach the kernel: 65 paths do not all stay as they are)
            assert not same_bits(call(ctx, case, without="stream")["rgb"], reference[i]["rgb"]), (i, case.name)
