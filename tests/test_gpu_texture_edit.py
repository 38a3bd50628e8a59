"""Texture edits of a resident scene (qa_scene_edit_texels[_device] / texmaps / textures / backdrop, Context.edit_*).

After the edits that turn blob A into blob B the context must be exactly where upload_scene(B) leaves a fresh one - same kernel name,
same bits in every later frame on every TEX kernel family, the edited blob back from download_scene - without a mesh build or a
device allocation; the float texel table the kernel of qa_texture_edit.hip rewrites equals the host's BuildTextures of B entry for
entry, for every rectangle shape, source alignment and stride its dword path and its texel-by-texel path can meet.  Every
comparison is bitwise.  tests/test_texture_edit_host.py pins the patched blobs to the oracle."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import bits, ensure_assets
from test_gpu_texture import _bad_rows, device_probe
from test_texture_host import cases, host_probe, probe_blob  # noqa: F401 (probe_blob: fixture)

import texture_edit_util as T

pytestmark = pytest.mark.gpu

QA_EINVAL, QA_ENOSCENE = -1, -5
CNT = ("samples", "casts_normal", "casts_shadow", "pixels")
SPP = 4
SCENES = {"small": ("custom_textures.xml", (80, 60)), "big": ("example_project7_object.xml", (80, 56))}
# the kernel families of tests/test_gpu_texture.py's texture-edge goldens: (scene, family, options, kernel name prefix)
FAMILIES = [
    ("small", "mega", dict(), "qa_integrate<RES=1,LIGHTS=1,TEX=1"),
    ("small", "stats", dict(), "qa_integrate<RES=1,LIGHTS=1,TEX=1"),
    ("small", "progressive", dict(), "qa_integrate<RES=1,LIGHTS=1,TEX=1"),
    ("big", "mega", dict(coop=0), "qa_integrate<RES=0,LIGHTS=1,TEX=1"),
    ("big", "mega", dict(coop=1, cs_cull=1), "qa_integrate_cs<LIGHTS=1,TEX=1,CULL=1"),
    ("big", "mega", dict(coop=1, cs_cull=0), "qa_integrate_cs<LIGHTS=1,TEX=1"),
    ("big", "staged", dict(coop=0), "staged"),
    ("big", "stats", dict(coop=0), "qa_integrate<RES=0,LIGHTS=1,TEX=1"),
    ("big", "progressive", dict(coop=0), "qa_integrate<RES=0,LIGHTS=1,TEX=1"),
]
DEFAULTS = dict(coop=1, cs_cull=1)


@pytest.fixture(scope="module")
def ctx():
    from qaray_amd import hip
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fresh():
    """The second context: only ever uploads."""
    from qaray_amd import hip
    c = hip.Context(0)
    yield c
    c.close()


_BLOBS = {}


def blobs(which):
    """-> (A, B, steps) of a scene, made once."""
    if which not in _BLOBS:
        from qaray_amd.host import load_scene_blob
        ensure_assets()
        scene, size = SCENES[which]
        a = load_scene_blob(scene, size=size)
        _BLOBS[which] = (a,) + T.make_b(a)
    return _BLOBS[which]


def same(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def render(c, family, region, spp=SPP):
    """-> (frame, counters, kernel name) of one frame of `family`."""
    c.reset_counters()
    if family == "progressive":
        with c.progressive(region, spp) as p:
            p.advance(1)
            p.advance(spp)
            out = p.read()
    else:
        out = c.render_region(region, spp, stats=family == "stats")
    cnt = c.counters()
    return out, {k: cnt[k] for k in CNT}, c.kernel_name()


def device():
    import torch
    return torch.device("cuda", 0)


def test_scene_b_has_every_kind_of_edit():
    for which in SCENES:
        a, b, steps = blobs(which)
        kinds = [s[0] for s in steps]
        assert kinds.count("texmaps") == 2 and {"texels_host", "texels_device", "textures", "backdrop"} <= set(kinds), (which, kinds)
        assert len(a) == len(b) and not np.array_equal(a, b)
    from qaray_amd import hip
    tex = hip.blob_table(blobs("small")[0], "textures")
    assert (64, 48) in {(int(t["width"]), int(t["height"])) for t in tex if t["type"] == 1}


@pytest.mark.parametrize("which,family,opts,kernel", FAMILIES, ids=[f"{w}-{f}-{'-'.join(f'{k}{v}' for k, v in o.items())}" for w, f, o, _ in FAMILIES])
def test_edits_leave_the_context_where_an_upload_of_b_does(ctx, fresh, which, family, opts, kernel):
    a, b, steps = blobs(which)
    region = (0, 0) + SCENES[which][1]
    try:
        for c in (ctx, fresh):
            for k, v in opts.items():
                c.set_option(k, v)
            c.set_pipeline("staged" if family == "staged" else "mega")
        ctx.upload_scene(a)
        frame_a, _, _ = render(ctx, family, region)
        before = ctx.scene_stats()
        assert before[3] == 0
        keep = []
        for n, step in enumerate(steps):
            keep.append(T.apply_step(ctx, step))
            st = ctx.scene_stats()
            assert st[0] == before[0], "an edit ran the per-mesh builder"
            assert st[1] == before[1], "an edit allocated device memory"
            assert st[3] == n + 1
            want = {"texels_host": step[3].size if step[0] == "texels_host" else 0, "texels_device": 0, "texmaps": 64, "textures": 56,
                    "backdrop": 32}[step[0]]
            assert st[2] == want, (step[0], st[2], want)
        assert np.array_equal(ctx.download_scene(), b)
        fresh.upload_scene(b)
        assert ctx.kernel_name() == fresh.kernel_name()
        f1, c1, n1 = render(ctx, family, region)
        f2, c2, n2 = render(fresh, family, region)
        assert n1 == n2 and (n1.startswith(kernel) or (family == "progressive" and "TEX=1" in n1)), (n1, n2)
        assert ("counting variant" in n1) == (family == "stats"), n1
        assert same(f1, f2), (which, family)
        assert c1 == c2
        assert not same(f1, frame_a), "the edits changed nothing"
        assert ctx.scene_stats()[:2] == before[:2]
    finally:
        for c in (ctx, fresh):
            for k, v in DEFAULTS.items():
                c.set_option(k, v)
            c.set_pipeline("auto")


def probe_equal(c, blob, wanted, table):
    """The device's texture tables of context c against the host's of `blob`: the (op, index, queries) of `table` that `wanted` picks."""
    c.synchronize()   # (the probe runs on the null stream)
    report, total = [], 0
    for op, index, q in table:
        if not wanted(op, index):
            continue
        d, h = device_probe(c, op, index, q), host_probe(blob, op, index, q)
        bad = _bad_rows(d, h)
        total += len(q)
        if len(bad):
            report.append(f"op {op} index {index}: {len(bad)} of {len(q)} differ, e.g. in {q[bad[0]][:9].tolist()} device {d[bad[0]][:3].tolist()} host {h[bad[0]][:3].tolist()}")
    assert not report, "\n".join(report[:20])
    return total


def test_texel_table_after_the_edits_equals_the_hosts(ctx):
    a, b, steps = blobs("small")
    ctx.upload_scene(a)
    keep = T.apply_steps(ctx, steps)
    total = probe_equal(ctx, b, lambda op, index: op in (1, 2, 4, 5), cases(b))
    assert total > 50000 and keep


def rect_cases(w, h):
    """(name, x0, y0, x1, y1, byte offset of the source, extra bytes per source row)"""
    ox0, oy0, ox1, oy1 = T.odd_rect(w, h)
    out = [("1x1", w // 2, h // 2, w // 2 + 1, h // 2 + 1, 0, 0), ("row", 0, h // 2, w, h // 2 + 1, 0, 0), ("column", w // 2, 0, w // 2 + 1, h, 0, 0),
           ("odd", ox0, oy0, ox1, oy1, 0, 0)]
    out += [(f"offset{k}", ox0, oy0, ox1, oy1, k, 0) for k in (1, 2, 3)]
    out += [("stride+1", ox0, oy0, ox1, oy1, 0, 1), ("whole", 0, 0, w, h, 0, 0), ("whole offset1", 0, 0, w, h, 1, 0), ("whole stride+1", 0, 0, w, h, 0, 1),
            ("last", w - 1, h - 1, w, h, 0, 0)]
    return out


@pytest.mark.parametrize("where", ["probe 1x7", "probe 7x1", "probe 3x5", "probe 8x8", "small 64x48"])
def test_rectangle_shapes(ctx, probe_blob, where):
    import torch
    from qaray_amd import hip
    scene, size = where.split()
    w, h = (int(v) for v in size.split("x"))
    work = np.array(probe_blob if scene == "probe" else blobs("small")[0], np.uint8, copy=True)
    tex = hip.blob_table(work, "textures")
    ti = [i for i in T.file_textures(work) if (int(tex[i]["width"]), int(tex[i]["height"])) == (w, h)][0]
    near = [i for i in (ti - 1, ti, ti + 1) if 0 <= i < len(tex)]
    table = [(op, index, q[:1500]) for op, index, q in cases(work) if (op == 1 and index in near) or (op == 2 and index == ti)]
    ctx.upload_scene(work)
    rng = np.random.default_rng(w * 100 + h)
    for name, x0, y0, x1, y1, off, extra in rect_cases(w, h):
        for source in ("host", "device"):
            rw, rh = x1 - x0, y1 - y0
            stride = 3 * rw + extra
            store = rng.integers(0, 256, off + rh * stride + 8).astype(np.uint8)
            if source == "host":
                px = np.lib.stride_tricks.as_strided(store[off:], (rh, rw, 3), (stride, 3, 1))
                arg = px
            else:
                dstore = torch.from_numpy(store).to(device())
                arg = dstore[off:].as_strided((rh, rw, 3), (stride, 3, 1))
                px = np.lib.stride_tricks.as_strided(store[off:], (rh, rw, 3), (stride, 3, 1))
                assert arg.data_ptr() % 4 == off % 4 and arg.stride(0) == stride
            hip.blob_texels(work, ti)[y0:y1, x0:x1] = px
            ctx.edit_texels(ti, arg, origin=(x0, y0))
            got = ctx.download_scene()
            assert np.array_equal(got, work), (where, name, source, np.nonzero(got != work)[0][:8])
            probe_equal(ctx, work, lambda op, index: True, table)


def test_frames_are_ordered_around_an_edit(ctx, fresh):
    """Render, edit, render on the context's stream with nothing waited for in between (device outputs, one synchronise at the end)."""
    import torch
    a, b, steps = blobs("small")
    size = SCENES["small"][1]
    region = (0, 0) + size
    n = size[0] * size[1]
    fresh.upload_scene(a)
    want_a = fresh.render_region(region, SPP)
    fresh.upload_scene(b)
    want_b = fresh.render_region(region, SPP)
    ctx.upload_scene(a)
    outs = [(torch.zeros(n * 3, dtype=torch.float32, device=device()), torch.zeros(n, dtype=torch.float32, device=device()),
             torch.zeros(n, dtype=torch.int32, device=device())) for _ in range(2)]
    dev_steps = [torch.from_numpy(s[3]).to(device()) if s[0] == "texels_device" else None for s in steps]
    torch.cuda.synchronize()
    ctx.render_region_device(region, SPP, *outs[0])
    for s, t in zip(steps, dev_steps):
        if t is not None:
            ctx.edit_texels(s[1], t, origin=s[2])
        else:
            T.apply_step(ctx, s)
    ctx.render_region_device(region, SPP, *outs[1])
    ctx.synchronize()
    got = [(o[0].cpu().numpy().reshape(size[1], size[0], 3), o[1].cpu().numpy().reshape(size[1], size[0]),
            o[2].cpu().numpy().view(np.uint32).reshape(size[1], size[0])) for o in outs]
    assert same(got[0], want_a), "the frame enqueued before the edits saw them"
    assert same(got[1], want_b), "the frame enqueued behind the edits missed them"


def test_device_source_may_be_overwritten_right_after_the_call(ctx, fresh):
    import torch
    from qaray_amd import hip
    a, _, _ = blobs("small")
    region = (0, 0) + SCENES["small"][1]
    ti = T.file_textures(a)[0]
    h, w = hip.blob_texels(a, ti).shape[:2]
    rng = np.random.default_rng(3)
    first, second = T.paint(rng, h, w), T.paint(rng, h, w)
    want = np.array(a, np.uint8, copy=True)
    hip.blob_texels(want, ti)[...] = first
    fresh.upload_scene(want)
    frame = fresh.render_region(region, SPP)
    ctx.upload_scene(a)
    s = torch.cuda.Stream(device())
    pinned = [torch.from_numpy(x).pin_memory() for x in (first, second)]
    t = torch.empty((h, w, 3), dtype=torch.uint8, device=device())
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        t.copy_(pinned[0], non_blocking=True)
        ctx.edit_texels(ti, t, stream=s.cuda_stream)
        t.copy_(pinned[1], non_blocking=True)
    assert ctx.scene_stats()[2] == 0
    assert same(ctx.render_region(region, SPP), frame)
    assert np.array_equal(ctx.download_scene(), want)
    s.synchronize()
    assert np.array_equal(t.cpu().numpy(), second)


def test_progressive_frame_goes_stale_and_restarts_in_place(ctx, fresh):
    from qaray_amd import hip
    a, b, steps = blobs("small")
    region = (0, 0) + SCENES["small"][1]
    fresh.upload_scene(b)
    want = fresh.render_region(region, 8)
    ctx.upload_scene(a)
    one_a = ctx.render_region(region, 4)
    with ctx.progressive(region, 8) as prog:
        prog.advance(4)
        keep = [T.apply_step(ctx, steps[0])]
        allocs = ctx.scene_stats()[1]
        with pytest.raises(hip.HipError) as e:
            prog.advance(8)
        assert e.value.code == QA_EINVAL and "edited" in str(e.value)
        assert same(prog.read(), one_a)
        keep += [T.apply_step(ctx, s) for s in steps[1:]]
        prog.restart()
        for s in (1, 4, 8):
            prog.advance(s)
        assert same(prog.read(), want)
        assert ctx.scene_stats()[1] == allocs
    assert same(ctx.render_region(region, 8), want) and keep


PHOTON_MAPS = ((2000, 20, 2.0), (300, 20, 3.0))


def test_photon_maps_are_dropped_by_a_texture_edit(ctx, tmp_path):
    """custom_photon.xml has a checker and no file texture: its maps go with an edit of the checker's colours, and those of a copy
    of the scene whose checker is a file texture with a texel edit."""
    from qaray_amd import hip
    from qaray_amd.host import SCENES_DIR, load_scene_blob
    size = (64, 48)
    region = (0, 0) + size
    text = open(os.path.join(SCENES_DIR, "custom_photon.xml")).read()
    assert text.count('texture="checkerboard"') == 1
    path = str(tmp_path / "custom_photon_file_texture.xml")
    open(path, "w").write(text.replace('texture="checkerboard"', 'texture="custom/bricks.ppm"'))
    for blob, kind in ((load_scene_blob("custom_photon.xml", size=size), "textures"), (load_scene_blob(path, size=size, asset_root=SCENES_DIR), "texels")):
        ctx.upload_scene(blob)
        ctx.build_photon_maps(*PHOTON_MAPS)
        ctx.photon_maps_info()
        ctx.render_region(region, 4)
        assert "photon-map gathers" in ctx.kernel_name()
        if kind == "texels":
            ti = T.file_textures(blob)[0]
            ctx.edit_texels(ti, T.paint(np.random.default_rng(1), 2, 3), origin=(1, 1))
        else:
            tex = hip.blob_table(blob.copy(), "textures")
            tex[0]["color1"] = np.float32(0.5)
            ctx.edit_textures(0, tex[:1])
        with pytest.raises(Exception, match="no photon maps"):
            ctx.photon_maps_info()
        ctx.render_region(region, 4)
        assert "photon-map gathers" not in ctx.kernel_name()


def test_refused_edits_change_nothing():
    import torch
    from qaray_amd import hip
    a, _, _ = blobs("small")
    region = (0, 0) + SCENES["small"][1]
    L = hip.lib()
    c = hip.Context(0)
    try:
        tex = hip.blob_table(a.copy(), "textures")
        maps = hip.blob_table(a.copy(), "texmaps")
        bg, env = (r.copy() for r in hip.blob_backdrop(a.copy()))
        ti = T.file_textures(a)[0]
        checker = [i for i in range(len(tex)) if tex[i]["type"] == 0][0]
        th, tw = hip.blob_texels(a, ti).shape[:2]
        px = np.zeros((2, 2, 3), np.uint8)
        for call in (lambda: c.edit_texels(ti, px), lambda: c.edit_texmaps(0, maps[:1]), lambda: c.edit_textures(0, tex[:1]),
                     lambda: c.edit_backdrop(bg, env), lambda: c.edit_texels(ti, torch.zeros((2, 2, 3), dtype=torch.uint8, device=device()))):
            with pytest.raises(hip.HipError) as e:
                call()
            assert e.value.code == QA_ENOSCENE
        c.upload_scene(a)
        frame_a = c.render_region(region, SPP)
        stats, name = c.scene_stats(), c.kernel_name()

        def refused(call):
            with pytest.raises(hip.HipError) as e:
                call()
            assert e.value.code == QA_EINVAL, e.value
            assert np.array_equal(c.download_scene(), a)
            assert c.scene_stats() == stats and c.kernel_name() == name
            assert same(c.render_region(region, SPP), frame_a)
            assert c.kernel_name() == name

        def raw(fn, *args):
            rc = fn(c._h, *args)
            if rc:
                raise hip.HipError(rc, L.qa_last_error().decode())

        dpx = torch.zeros((2, 2, 3), dtype=torch.uint8, device=device())
        wide = np.zeros((1, tw + 1, 3), np.uint8)
        for src in (lambda v: v, lambda v: torch.from_numpy(v).to(device())):
            refused(lambda: c.edit_texels(checker, src(px)))                         # a checker texture
            refused(lambda: c.edit_texels(ti, src(px), origin=(tw - 1, 0)))          # beyond the texture, to the right
            refused(lambda: c.edit_texels(ti, src(px), origin=(0, th - 1)))          # ... below
            refused(lambda: c.edit_texels(ti, src(px), origin=(-1, 0)))
            refused(lambda: c.edit_texels(ti, src(wide)))
            refused(lambda: c.edit_texels(len(tex), src(px)))                        # a texture index beyond the table
        for fn, args in ((L.qa_scene_edit_texels, ()), (L.qa_scene_edit_texels_device, (None,))):
            ptr = px.ctypes.data if not args else dpx.data_ptr()
            refused(lambda: raw(fn, ti, 1, 0, 1, 2, ptr, 6, *args))                  # x1 <= x0
            refused(lambda: raw(fn, ti, 0, 1, 2, 1, ptr, 6, *args))                  # y1 <= y0
            refused(lambda: raw(fn, ti, 0, 0, 2, 2, ptr, 5, *args))                  # a short stride
            refused(lambda: raw(fn, ti, 0, 0, 2, 2, None, 6, *args))                 # a null source
        for field, value in (("width", tw + 1), ("height", th - 1), ("type", 0), ("off_texels", int(tex[ti]["off_texels"]) + 3)):
            r = tex[ti:ti + 1].copy()
            r[0][field] = value
            refused(lambda: c.edit_textures(ti, r))
        r = tex[checker:checker + 1].copy()
        r[0]["type"] = 1
        refused(lambda: c.edit_textures(checker, r))
        refused(lambda: c.edit_textures(len(tex), tex[:1]))
        for value in (len(tex), -2):
            r = maps[:1].copy()
            r[0]["texture"] = value
            refused(lambda: c.edit_texmaps(0, r))
        refused(lambda: c.edit_texmaps(len(maps) - 1, maps[:2]))
        for which in (0, 1):
            r = [bg.copy(), env.copy()]
            r[which]["texmap"] = -1 if r[which]["texmap"] >= 0 else 0
            refused(lambda: c.edit_backdrop(*r))
            refused(lambda: c.edit_backdrop(**{("background", "environment")[which]: r[which]}))
    finally:
        c.close()


def test_edited_frames_do_not_depend_on_scratch_contents():
    from qaray_amd import hip
    a, b, steps = blobs("small")
    region = (0, 0) + SCENES["small"][1]
    c = hip.Context(0)
    try:
        c.upload_scene(a)
        c.render_region(region, SPP)
        keep = T.apply_steps(c, steps)
        frames = []
        for pattern in (0x00000000, 0xFFFFFFFF, 0x3F800000):
            c.scrub_scratch(pattern)
            frames.append(c.render_region(region, SPP))
        assert same(frames[0], frames[1]) and same(frames[0], frames[2]) and keep
    finally:
        c.close()
