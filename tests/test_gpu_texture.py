"""The device build of the texture path (qaray_amd/csrc/hip/qa_texture_dev.h) against its host build, bit for bit, on the MI355X:
qa_test_texture_device runs one query per lane on the tables of the uploaded scene, qa_test_texture_host the same source on the CPU
with the tables BuildScene makes.  tests/test_texture_host.py pins the host build to the oracle on the same inputs (edge sets:
out-of-range uv up to +-2^31 and beyond, infinities, NaN, denormal and zero differentials, 1-texel-wide textures, the environment's
poles; and seeded random sweeps), so together they pin every texture lookup of the TEX kernels.  A device whose (int) conversion
clamps (v_cvt_i32_f32) instead of giving x86's INT_MIN from 2^31 on fails here.  NaN equals NaN; payloads are not compared."""
import ctypes as C

import numpy as np
import pytest

from test_texture_host import NIN, NOUT, cases, host_probe, probe_blob, queries  # noqa: F401 (probe_blob: fixture)

pytestmark = pytest.mark.gpu


def device_probe(ctx, op, index, q):
    from qaray_amd import hip
    L = hip.lib()
    L.qa_test_texture_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    q = np.ascontiguousarray(q, np.float32)
    out = np.zeros((len(q), NOUT), np.float32)
    rc = L.qa_test_texture_device(ctx._h, op, index, len(q), q.ctypes.data, out.ctypes.data)
    assert rc == 0, L.qa_last_error()
    return out


def _bad_rows(d, h):
    return np.nonzero(~np.all((d.view(np.uint32) == h.view(np.uint32)) | (np.isnan(d) & np.isnan(h)), axis=1))[0]


def test_device_texture_path_equals_host(probe_blob):
    from qaray_amd import hip
    ctx = hip.Context(0)
    try:
        ctx.upload_scene(probe_blob)
        report, total = [], 0
        for op, index, q in cases(probe_blob):
            d, h = device_probe(ctx, op, index, q), host_probe(probe_blob, op, index, q)
            bad = _bad_rows(d, h)
            total += len(q)
            for r in bad[:3]:
                report.append(f"op {op} index {index}: in {q[r][:9].tolist()} device {d[r][:3].tolist()} host {h[r][:3].tolist()}")
            if len(bad):
                report.append(f"op {op} index {index}: {len(bad)} of {len(q)} queries differ")
        # the conversion helper itself (op 9) on every 4099th float bit pattern
        x = np.arange(0, 1 << 32, 4099, dtype=np.uint64).astype(np.uint32).view(np.float32)
        q = queries(a=np.stack([x, x, x], axis=1))
        d, h = device_probe(ctx, 9, 0, q), host_probe(probe_blob, 9, 0, q)
        bad = _bad_rows(d, h)
        if len(bad):
            report.append(f"op 9: {len(bad)} of {len(q)} conversions differ, e.g. {x[bad[:3]].tolist()}: device "
                          f"{d[bad[:3], 0].view(np.int32).tolist()} host {h[bad[:3], 0].view(np.int32).tolist()}")
        print("\n".join(report) or f"{total} texture queries and {len(q)} conversions: device == host")
        assert not report, "\n".join(report[:40])
    finally:
        ctx.close()


# ---- the texture-edge goldens on every TEX family ------------------------------------------------------------------------------
# tests/golden/texedge_*: a floor whose lookups cross +-2^31, a checker wall at grazing angles, a textured sphere and mesh, textured
# background and environment, rendered by the reference.  Bounce 0 (one path segment): the colours reach 1e21 there, and with more
# segments the kernels' front-to-back sum and the reference's nested one round differently - a tolerance would mean nothing.
# The meshes are fans of 24 and 4 x 130 triangles (LDS-resident; global memory with the 4-wide tree), texture vertices up to 1e10.
FAMILIES = [  # (golden, family, set-up, kernel name prefix)
    ("texedge_small_48x36_2spp_bounce0", "mega", dict(), "qa_integrate<RES=1,LIGHTS=1,TEX=1"),
    ("texedge_small_48x36_2spp_bounce0", "stats", dict(), "qa_integrate<RES=1,LIGHTS=1,TEX=1"),
    ("texedge_small_48x36_2spp_bounce0", "progressive", dict(), "qa_integrate<RES=1,LIGHTS=1,TEX=1"),
    ("texedge_big_48x36_2spp_bounce0", "mega", dict(coop=0), "qa_integrate<RES=0,LIGHTS=1,TEX=1"),
    ("texedge_big_48x36_2spp_bounce0", "mega", dict(coop=1, cs_cull=1), "qa_integrate_cs<LIGHTS=1,TEX=1,CULL=1"),
    ("texedge_big_48x36_2spp_bounce0", "mega", dict(coop=1, cs_cull=0), "qa_integrate_cs<LIGHTS=1,TEX=1"),
    ("texedge_big_48x36_2spp_bounce0", "staged", dict(coop=0), "staged"),
    ("texedge_big_48x36_2spp_bounce0", "stats", dict(coop=0), "qa_integrate<RES=0,LIGHTS=1,TEX=1"),
    ("texedge_big_48x36_2spp_bounce0", "progressive", dict(coop=0), "qa_integrate<RES=0,LIGHTS=1,TEX=1"),
]


@pytest.mark.parametrize("golden,family,opts,kernel", FAMILIES, ids=[f"{g.split('_')[1]}-{f}-{'-'.join(f'{k}{v}' for k, v in o.items())}"
                                                                       for g, f, o, _ in FAMILIES])
def test_texture_edge_golden_on_every_tex_family(golden, family, opts, kernel):
    from conftest import bits, golden_blob, load_golden
    from qaray_amd import hip
    rgb, depth, ns, meta = load_golden(golden)
    blob = golden_blob(meta)
    region, spp = tuple(meta["crop"]), meta["spp_min"]
    c = hip.Context(0)
    try:
        for k, v in opts.items():
            c.set_option(k, v)
        c.upload_scene(blob)
        c.set_pipeline("staged" if family == "staged" else "mega")
        c.reset_counters()
        if family == "progressive":
            with c.progressive(region, spp, spp_max=meta["spp_max"], max_bounce=meta["bounce"]) as p:
                p.advance(1)
                p.advance(spp)
                out = p.read()
        else:
            out = c.render_region(region, spp, max_bounce=meta["bounce"], spp_max=meta["spp_max"], stats=family == "stats")
        cnt, name = c.counters(), c.kernel_name()
    finally:
        c.close()
    assert name.startswith(kernel) or (family == "progressive" and "TEX=1" in name), name
    assert ("counting variant" in name) == (family == "stats"), name
    g_rgb, g_depth, g_ns = out[:3]
    assert np.array_equal(g_ns, ns)
    assert np.array_equal(bits(g_depth), bits(depth))
    assert (cnt["samples"], cnt["casts_normal"], cnt["casts_shadow"]) == (meta["samples"], meta["casts_normal"], meta["casts_shadow"])
    bad = np.argwhere((bits(g_rgb) != bits(rgb)) & ~(np.isnan(g_rgb) & np.isnan(rgb)))   # (NaN payloads: x86 and gfx950 differ)
    assert len(bad) == 0, f"{len(bad)} radiance values differ, first at {bad[0].tolist()}: {g_rgb[tuple(bad[0])]} vs {rgb[tuple(bad[0])]}"
