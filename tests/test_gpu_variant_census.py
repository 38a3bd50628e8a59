"""Census of the integrator instances the library ships: one row per instance, each run on a small synthetic scene that
selects it, and compared with the oracle and with its sibling variants.

ROWS holds one row per shipped kernel instance (tests/test_variant_census_closure.py checks, without a GPU, that its
instances are exactly the integrator kernels in the built objects):
  * qa_integrate<RES, LIGHTS, TEX, AREA, STATS, PHOTON>   36 rows  (PickKernel, qa_photon.hip PickPmKernel)
  * qa_integrate_cs<LIGHTS, TEX, CULL, MANY, AREA>        12 rows  (PickCs)
  * qa_integrate_cs_resume<LIGHTS, TEX, CULL, MANY, AREA>  6 rows  (PickCsResume: progressive passes)
  * the staged pipeline: wf_logic<TEX>, with wf_init / wf_cull / wf_trace / wf_redo on the first of its two rows.
Every row: kernel_name() names exactly the instance; an odd frame (partial 8x8 tiles), >= 2 spp, some rows adaptive;
sample counts, depth and cast counters equal the oracle's, radiance within test_gpu_parity.py's tolerances; and bit for bit
equal to a sibling where one exists (cooperative == coop=0 megakernel, STATS == plain, resume == one-shot cooperative,
staged == megakernel).  The counting rows of scenes without lights also match the oracle's BVH-node / triangle-test counters
(with lights the reference's shadow walk in a mesh goes on past its first hit, the kernels stop: see test_gpu_parity.py).
A row whose cell no scene can reach would carry `unreachable` (the reason) instead of a scene: today every cell is reached.
"""
import os
from collections import namedtuple

import numpy as np
import pytest

from conftest import bits

pytestmark = pytest.mark.gpu

W, H = 52, 37                 # partial tiles on both axes
RMSE_TOL, MAXABS_TOL = 1e-6, 1e-4   # test_gpu_parity.py
PHOTON, CAUSTICS = (2000, 20, 0.5), (200, 20, 1.0)

# lights: a point light (+ ambient); tex: textured floor / sphere / environment; area: a point light of size 1; big: a mesh of
# 4608 triangles (not LDS-resident); many: 6 shadow-casting lights (> QA_CS_LIGHT_BATCH); nodes: 16 extra spheres (> 12
# nodes); overflow: a node whose transform overflows the instance-culling constants (plan.csCullOk = false)
Scene = namedtuple("Scene", "lights tex area big many nodes overflow")
Row = namedtuple("Row", "instances scene call spp spp_max name unreachable")


def _b(v):
    return "true" if v else "false"


def _rows():
    rows = []
    shadings = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 0, 1), (1, 1, 1)]   # (LIGHTS, TEX, AREA) as PickShading has them
    for res in (1, 0):
        for (l, t, a) in shadings:
            for photon in (0, 1):
                if photon and not l:
                    continue   # (the photon variants all have LIGHTS=1: a map needs a light to emit from)
                for stats in (0, 1):
                    adaptive = (res + l + t + a + photon) % 2 == 1
                    name = f"qa_integrate<RES={res},LIGHTS={l},TEX={t},AREA={a}>"
                    name += " + photon-map gathers (PHOTON=1)" if photon else ""
                    name += " counting variant (STATS=1, reference tree)" if stats else ""
                    rows.append(Row((f"qa::qa_integrate<{_b(res)}, {_b(l)}, {_b(t)}, {_b(a)}, {_b(stats)}, {_b(photon)}>",),
                                    Scene(l, t, a, not res, 0, 0, 0), ("photon" if photon else "mega") + ("_stats" if stats else ""),
                                    2, 6 if adaptive else 2, name, None))
    # PickCs's table: (LIGHTS, TEX, CULL, MANY, AREA)
    cs = [(0, 0, 0, 0, 0), (0, 1, 0, 0, 0), (1, 0, 0, 0, 0), (1, 1, 0, 0, 0), (0, 0, 1, 0, 0), (0, 1, 1, 0, 0), (1, 0, 1, 0, 0),
          (1, 1, 1, 0, 0), (1, 0, 1, 1, 0), (1, 1, 1, 1, 0), (1, 0, 1, 0, 1), (1, 1, 1, 0, 1)]
    for (l, t, cull, many, a) in cs:
        # untextured scenes cull from 13 nodes on; textured ones always, unless the culling constants overflow
        scene = Scene(l, t, a, 1, many, int(cull and not t and not many and not a), int(t and not cull))
        suffix = f"LIGHTS={l},TEX={t},CULL={cull}" + (",MANY=1" if many else "") + (",AREA=1" if a else "")
        args = f"{_b(l)}, {_b(t)}, {_b(cull)}, {_b(many)}, {_b(a)}>"
        adaptive = (l + t + cull) % 2 == 0
        rows.append(Row(("qa::qa_integrate_cs<" + args,), scene, "cs", 3, 7 if adaptive else 3, f"qa_integrate_cs<{suffix}>", None))
        if not t:
            rows.append(Row(("qa::qa_integrate_cs_resume<" + args,), scene, "resume", 3, 7 if adaptive else 3,
                            f"qa_integrate_cs_resume<{suffix}>", None))
    rows.append(Row(("qa::wf_logic<false>", "qa::wf_init", "qa::wf_cull", "qa::wf_trace", "qa::wf_redo"), Scene(1, 0, 0, 1, 0, 0, 0),
                    "staged", 2, 6, "staged: wf_logic + wf_cull + wf_trace + wf_redo", None))
    rows.append(Row(("qa::wf_logic<true>",), Scene(1, 1, 0, 1, 0, 0, 0), "staged", 3, 3, "staged: wf_logic + wf_cull + wf_trace + wf_redo", None))
    return rows


ROWS = _rows()


def _row_id(r):
    return r.instances[0].replace("qa::", "").replace(" ", "").replace("true", "1").replace("false", "0")


def write_scene(d, sc):
    """The row's scene under directory d: a floor, a sphere, a height-field mesh with texture vertices, and the switches."""
    n = 48 if sc.big else 3
    with open(os.path.join(d, "mesh.obj"), "w") as f:
        for j in range(n + 1):
            for i in range(n + 1):
                x, y = -4 + 8 * i / n, -4 + 8 * j / n
                f.write("v %.7g %.7g %.7g\nvt %.7g %.7g\n" % (x, y, 1.2 + 0.6 * np.sin(1.3 * x) * np.cos(0.9 * y), i / n, j / n))
        for j in range(n):
            for i in range(n):
                a, b, c, e = j * (n + 1) + i + 1, j * (n + 1) + i + 2, (j + 1) * (n + 1) + i + 2, (j + 1) * (n + 1) + i + 1
                f.write("f %d/%d %d/%d %d/%d\nf %d/%d %d/%d %d/%d\n" % (a, a, b, b, c, c, a, a, c, c, e, e))
    with open(os.path.join(d, "tex.ppm"), "wb") as f:
        f.write(b"P6 8 8 255\n" + bytes((37 * k + 11 * (k // 24)) % 256 for k in range(8 * 8 * 3)))
    tex = sc.tex
    floor_diffuse = ('<diffuse r="0.7" g="0.7" b="0.6" texture="checkerboard"><color1 r="0.2" g="0.2" b="0.3"/><color2 r="0.8" g="0.7" b="0.6"/>'
                     '<scale value="0.2"/></diffuse>' if tex else '<diffuse r="0.7" g="0.7" b="0.6"/>')
    m = ['<material type="blinn" name="floor">%s<specular value="0.2"/><glossiness value="15"/><reflection value="0.2"/>'
         '<emission value="0.05"/></material>' % floor_diffuse,
         '<material type="blinn" name="ball"><diffuse r="0.8" g="0.3" b="0.2"%s/><specular value="0.5"/><glossiness value="40"/>'
         '<emission value="0.1"/></material>' % (' texture="tex.ppm"' if tex else ""),
         '<material type="blinn" name="mesh"><diffuse r="0.3" g="0.6" b="0.8"%s/><specular value="0.4"/><glossiness value="25"/>'
         '<reflection value="0.3"/><emission value="0.08"/></material>' % (' texture="tex.ppm"' if tex else ""),
         '<material type="blinn" name="glass"><diffuse value="0"/><specular value="0.8"/><glossiness value="60"/>'
         '<refraction value="0.9" index="1.5"/></material>']
    objs = ['<object type="plane" name="floor" material="floor"><scale value="30"/></object>',
            '<object type="sphere" name="ball" material="ball"><scale value="2"/><rotate angle="30" x="1" y="0.5"/><translate x="-5" y="1" z="2"/></object>',
            '<object type="sphere" name="lens" material="glass"><scale value="1.2"/><translate x="4.5" y="-3" z="1.5"/></object>',
            '<object type="obj" name="mesh.obj" material="mesh"><rotate angle="20" z="1"/><translate x="1" y="2" z="0"/></object>']
    if sc.nodes:
        for k in range(16):
            a = 2 * np.pi * k / 16
            objs.append('<object type="sphere" name="n%d" material="%s"><scale value="0.6"/><translate x="%.6g" y="%.6g" z="0.6"/></object>'
                        % (k, "ball" if k % 2 else "floor", 9 * np.cos(a), 9 * np.sin(a)))
    if sc.overflow:
        # a sphere squashed to a disc 1e22 wide and 1e-22 thick: its condition number (1e44) overflows the culling constants
        objs.append('<object type="sphere" name="disc" material="floor"><scale x="1e22" y="1e-22" z="1"/><translate y="40" z="-50"/></object>')
    lights = []
    if sc.lights:
        lights += ['<light type="ambient" name="amb"><intensity value="0.1"/></light>',
                   '<light type="point" name="p0"><intensity value="40"/><position x="3" y="-8" z="12"/></light>']
    if sc.area:
        lights.append('<light type="point" name="area"><intensity value="30"/><position x="-6" y="-4" z="10"/><size value="1"/></light>')
    if sc.many:
        for k in range(5):
            lights.append('<light type="point" name="m%d"><intensity value="8"/><position x="%d" y="%d" z="9"/></light>' % (k, 4 * k - 8, 6 - 3 * k))
    env = '<environment value="0.5" texture="tex.ppm"/>' if tex else '<environment value="0.3"/>'
    xml = ("<xml><scene>" + '<background r="0.3" g="0.4" b="0.5"/>' + env + "".join(objs) + "".join(m) + "".join(lights) + "</scene>"
           '<camera><position x="1" y="-20" z="9"/><target x="0" y="0" z="1"/><up x="0" y="0" z="1"/><fov value="45"/>'
           "<width value=\"104\"/><height value=\"74\"/></camera></xml>")
    path = os.path.join(d, "census.xml")
    open(path, "w").write(xml)
    return path


_blobs = {}


@pytest.fixture(scope="module")
def blob_of(tmp_path_factory):
    def get(sc):
        if sc not in _blobs:
            from qaray_amd.host import load_scene_blob
            d = str(tmp_path_factory.mktemp("census"))
            _blobs[sc] = load_scene_blob(write_scene(d, sc), size=(W, H), asset_root=d)
        return _blobs[sc]
    return get


def _render(blob, row, call, coop=1):
    """-> (rgb, depth, ns), counters, kernel_name() after the frame, photon maps (or None); on a fresh context."""
    from qaray_amd import hip
    c = hip.Context(0)
    try:
        c.set_option("coop", coop)
        c.upload_scene(blob)
        c.set_pipeline("staged" if call == "staged" else "mega")
        maps = None
        if call.startswith("photon"):
            c.build_photon_maps(PHOTON, CAUSTICS)
            maps = (c.download_photon_map(0), c.download_photon_map(1))
        c.reset_counters()
        region = (0, 0, W, H)
        if call == "resume":
            with c.progressive(region, row.spp, spp_max=row.spp_max) as p:
                p.advance(1)
                p.advance(row.spp_max)
                out = p.read()
        else:
            out = c.render_region(region, row.spp, spp_max=row.spp_max, stats=call.endswith("_stats"))
        return tuple(out[:3]), c.counters(), c.kernel_name(), maps
    finally:
        c.close()


def _same(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("row", [r for r in ROWS if r.unreachable is None], ids=_row_id)
def test_variant_against_oracle_and_siblings(blob_of, row):
    from oracle import binding as oracle
    blob = blob_of(row.scene)
    cs = row.call in ("cs", "resume")
    out, cnt, name, maps = _render(blob, row, row.call, coop=1 if cs else 0)
    if row.call == "staged":
        assert name.startswith(row.name), name
    else:
        assert name == row.name, name
    photon = None
    if maps is not None:
        photon = (oracle.photon_params(PHOTON, CAUSTICS), maps[0], maps[1])
    o_rgb, o_depth, o_ns, o_cnt = oracle.render(blob, (0, 0, W, H), row.spp, spp_max=row.spp_max, photon=photon)
    rgb, depth, ns = out
    assert ns.min() >= row.spp
    assert np.array_equal(ns, o_ns) and np.array_equal(bits(depth), bits(o_depth))
    assert (cnt["samples"], cnt["casts_normal"], cnt["casts_shadow"]) == (o_cnt.samples, o_cnt.casts_normal, o_cnt.casts_shadow)
    assert np.isfinite(rgb).all() == np.isfinite(o_rgb).all()
    scale = max(1.0, float(np.abs(o_rgb[np.isfinite(o_rgb)]).max()))
    diff = float(np.nanmax(np.abs(rgb.astype(np.float64) - o_rgb)))
    err = float(np.sqrt(np.mean((np.nan_to_num(rgb).astype(np.float64) - np.nan_to_num(o_rgb)) ** 2)))
    print(f"census {row.instances[0]} | {name} | max |rgb - oracle| {diff:.3g}")
    assert diff <= MAXABS_TOL * scale and err <= RMSE_TOL * scale
    if row.call.endswith("_stats") and not row.scene.lights:
        assert (cnt["bvh_nodes"], cnt["tri_tests"]) == (o_cnt.bvh_nodes, o_cnt.tri_tests)
    # siblings, bit for bit
    if row.call in ("mega_stats", "photon_stats"):
        sib = _render(blob, row, row.call[:-len("_stats")], coop=0)
        assert sib[2] == row.name.replace(" counting variant (STATS=1, reference tree)", ""), sib[2]
    elif row.call == "cs":
        sib = _render(blob, row, "mega", coop=0)
        assert sib[2].startswith("qa_integrate<RES=0,"), sib[2]
    elif row.call == "resume":
        sib = _render(blob, row, "cs", coop=1)
        assert sib[2] == row.name.replace("_resume", ""), sib[2]
    elif row.call == "staged":
        sib = _render(blob, row, "mega", coop=0)
    else:
        return
    assert _same(out, sib[0])
    assert all(cnt[k] == sib[1][k] for k in ("samples", "casts_normal", "casts_shadow"))
