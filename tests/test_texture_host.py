"""The texture path (qaray_amd/csrc/hip/qa_texture_dev.h) compiled for the host, against the oracle's own texture functions, bit for
bit: tileClamp, checker and bilinear lookups, the 32-tap elliptical filter, texture transforms, the environment lookup and the uv
differentials of planes, spheres and triangles (qa_test_texture_host vs oracle/qa_oracle.c qa_oracle_texture_probe, the same op
numbers: include/qaray_hip.h).  The host hook builds its tables with BuildScene, so the per-texel x / 255.0f floats and the 31 tap
offsets of an upload are under test too.  The inputs are edge sets - out-of-range uv up to +-2^31 and beyond, infinities and NaN,
denormal and zero differentials, 1-texel-wide textures, grazing differentials, the environment's poles - and seeded random sweeps.
tests/test_gpu_texture.py runs the same inputs through the device build.  NaN equals NaN; payloads are not compared."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_device_math import same_bits

NIN, NOUT = 16, 9
F32 = np.float32


def _f(*v):
    return np.array(v, F32)


def _nb(x, n=1):
    """x and its n float neighbours on either side."""
    x = F32(x)
    out = [x]
    lo = hi = x
    for _ in range(n):
        lo, hi = np.nextafter(lo, F32(-np.inf)), np.nextafter(hi, F32(np.inf))
        out += [lo, hi]
    return out


def _uv_edges():
    ints = []
    for k in (1, 2, 3, 7, 255, 1024, 65537, 1 << 23, (1 << 24) - 1, 1 << 24):
        ints += _nb(k) + _nb(-k)
    v = [0.0, -0.0, *_nb(0.5), *_nb(-0.5), F32(1) - F32(2 ** -24), -F32(2 ** -24), -F32(2 ** -149), F32(2 ** -149), F32(1e-39),
         F32(-1e-39), 0.25, 0.75, 1.0, -1.0, 2147483520.0, 2 ** 31, -2 ** 31, 2 ** 31 + 256, -(2 ** 31 + 256), 3e9, -3e9, 1e10, -1e10,
         np.finfo(F32).max, -np.finfo(F32).max, np.inf, -np.inf, np.nan, *ints]
    return np.array(v, F32)


UV = _uv_edges()
D_EDGES = [(0, 0, 0), (0.0, -0.0, 0.0), (-0.0, -0.0, -0.0), (1e-45, 0, 0), (0, -1e-45, 0), (1e10, 0, 0), (0, -1e10, 3),
           (np.inf, 0, 0), (0, -np.inf, 0), (np.nan, 0, 0), (0.01, 0.02, 0), (-0.3, 0.2, 0), (2.0, -3.0, 0)]


def queries(n=0, **cols):
    """float32 [n, 16] from named column blocks: a (0..2), b (3..5), c (6..8), d (9..11), e (12..14), flag (15)."""
    at = dict(a=0, b=3, c=6, d=9, e=12, flag=15)
    n = n or max(len(np.atleast_2d(v)) for v in cols.values())
    q = np.zeros((n, NIN), F32)
    for k, v in cols.items():
        v = np.asarray(v, F32)
        width = 1 if k == "flag" else 3
        q[:, at[k]:at[k] + width] = v.reshape(-1, width) if v.ndim else v
    return q


def uv_grid(rng, n_random=4000):
    """Every pair of the uv edge set (x, y) with z from a short list, plus seeded random coordinates of every magnitude."""
    x, y = np.meshgrid(UV, UV)
    z = np.resize(_f(0.0, -0.0, 0.5, 3e9, np.nan, -1.0), x.size)
    g = np.stack([x.ravel(), y.ravel(), z], axis=1)
    mag = F32(10.0) ** rng.uniform(-8, 11, (n_random, 3)).astype(F32)
    r = (rng.choice(_f(-1, 1), (n_random, 3)) * mag).astype(F32)
    return np.concatenate([g, r])


# ---- the probe scene ------------------------------------------------------------------------------
TEX_SIZES = [(1, 1), (1, 7), (7, 1), (3, 5), (8, 8)]
TRANSFORMS = ["", '<scale value="1e-10"/>', '<rotate angle="33" z="1"/><translate x="0.3" y="-2.7" z="0.5"/>']


def write_probe_scene(d):
    """A scene whose texture tables hold every case of the probes: file textures of 1x1, 1x7, 7x1, 3x5 and 8x8 texels (0 and 255
    among them), a checker, each under an identity map, a scale of 1e-10 and a rotation plus translation; a map whose file is
    missing (texture -1); textured background and environment; a mesh with texture vertices.  -> path of the XML."""
    rng = np.random.default_rng(11)
    for w, h in TEX_SIZES:
        px = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        px.reshape(-1, 3)[0] = (0, 255, 0)
        px.reshape(-1, 3)[-1] = (255, 0, 255)
        with open(os.path.join(d, f"t{w}x{h}.ppm"), "wb") as f:
            f.write(b"P6\n%d %d\n255\n" % (w, h) + px.tobytes())
    with open(os.path.join(d, "mesh.obj"), "w") as f:
        f.write("v -1 -1 0\nv 1 -1 0.2\nv 1 1 -0.3\nv -1 1 0\nv 0 0 1.5\n")
        f.write("vt 0 0\nvt 3e9 -2\nvt 1e10 1e10\nvt -0.5 0.25\nvt 0.5 0.5\n")
        f.write("f 1/1 2/2 5/5\nf 2/2 3/3 5/5\nf 3/3 4/4 5/5\nf 4/4 1/1 5/5\nf 1/1 3/3 2/2\n")
    mats, objs = [], []
    k = 0
    kinds = [f't{w}x{h}.ppm' for w, h in TEX_SIZES] + ["checkerboard"]
    for tex in kinds:
        for xf in TRANSFORMS:
            inner = '<color1 r="0.1" g="0.2" b="0.3"/><color2 r="0.9" g="0.8" b="0.7"/>' if tex == "checkerboard" else ""
            mats.append(f'<material type="blinn" name="m{k}"><diffuse r="0.9" g="0.5" b="0.2" texture="{tex}">{inner}{xf}</diffuse></material>')
            objs.append(f'<object type="sphere" name="s{k}" material="m{k}"><translate x="{3 * k}" y="0" z="0"/></object>')
            k += 1
    mats.append('<material type="blinn" name="missing"><diffuse r="0.5" g="0.5" b="0.5" texture="missing.ppm"/></material>')
    objs.append('<object type="plane" name="floor" material="missing"><scale value="5"/></object>')
    objs.append('<object type="obj" name="mesh.obj" material="m0"/>')
    xml = ("<xml><scene>" + '<background r="0.3" g="0.4" b="0.5" texture="t3x5.ppm"/>'
           '<environment r="1" g="0.5" b="0.25" texture="t8x8.ppm"><rotate angle="10" x="1"/></environment>'
           + "".join(objs) + "".join(mats) +
           '<light type="point" name="p"><intensity value="10"/><position x="0" y="-5" z="5"/></light></scene>'
           '<camera><position x="0" y="-20" z="5"/><target x="0" y="0" z="0"/><up x="0" y="0" z="1"/><fov value="40"/>'
           '<width value="32"/><height value="24"/></camera></xml>')
    path = os.path.join(d, "probe.xml")
    open(path, "w").write(xml)
    return path


_HDR = dict(num_meshes=140, num_texmaps=156, num_textures=160, off_meshes=176, off_texmaps=208, off_textures=216)
TEXMAP = np.dtype([("itm", "<f4", 9), ("pos", "<f4", 3), ("texture", "<i4"), ("pad", "<i4", 3)])
TEXTURE = np.dtype([("type", "<i4"), ("width", "<i4"), ("height", "<i4"), ("pad0", "<i4"), ("color1", "<f4", 3), ("color2", "<f4", 3),
                    ("off_texels", "<u8"), ("pad1", "<u8")])


def tables(blob):
    """-> (textures, texmaps, faces of mesh 0) of a flat blob (include/qa_flat_scene.h)."""
    b = np.asarray(blob, np.uint8)
    u32 = lambda off: int(np.frombuffer(b, "<u4", 1, off)[0])
    u64 = lambda off: int(np.frombuffer(b, "<u8", 1, off)[0])
    tex = np.frombuffer(b, TEXTURE, u32(_HDR["num_textures"]), u64(_HDR["off_textures"]))
    maps = np.frombuffer(b, TEXMAP, u32(_HDR["num_texmaps"]), u64(_HDR["off_texmaps"]))
    nmesh = u32(_HDR["num_meshes"])
    faces = int(np.frombuffer(b, "<u4", 1, u64(_HDR["off_meshes"]) + 24)[0]) if nmesh else 0
    return tex, maps, faces


@pytest.fixture(scope="module")
def probe_blob(tmp_path_factory):
    from qaray_amd.host import load_scene_blob
    d = str(tmp_path_factory.mktemp("texprobe"))
    return load_scene_blob(write_probe_scene(d), size=(32, 24), asset_root=d)


def host_probe(blob, op, index, q):
    from qaray_amd import hip
    L = hip.lib()
    L.qa_test_texture_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    q = np.ascontiguousarray(q, F32)
    out = np.zeros((len(q), NOUT), F32)
    b = None if blob is None else np.ascontiguousarray(blob, np.uint8)
    rc = L.qa_test_texture_host(None if b is None else b.ctypes.data, op, index, len(q), q.ctypes.data, out.ctypes.data)
    assert rc == 0, rc
    return out


# ---- the cases: (op, index, queries), shared with tests/test_gpu_texture.py ------------------------
def _directions(rng, n):
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    axes = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (-0.0, -0.0, 1), (0.0, -0.0, -1), (-0.0, 1, 0),
            (1, -0.0, 0), (-0.0, 0.0, -0.0), (1e-30, 1e-30, 1), (-1e-38, 1e-45, -1), (0.6, 0.8, 0), (np.nan, 0, 1), (0, 0, np.inf)]
    return np.concatenate([np.array(axes, F32), d.astype(F32)])


def _diff_cases(rng, n):
    """Ray origins and differential directions: random camera-like ones plus the edges - dx parallel to the plane (dot = 0), a
    denormal dot, a differential that points away (t_x < 0), zero and NaN directions."""
    o = np.concatenate([rng.uniform(-3, 3, (n, 2)), rng.uniform(0.5, 6, (n, 1))], axis=1).astype(F32)
    dx = rng.normal(size=(n, 3)).astype(F32)
    dy = (dx + rng.normal(scale=1e-3, size=(n, 3))).astype(F32)
    edge_d = np.array([(1, 0, 0), (0, 1, -0.0), (1, 0, 1e-45), (0, 1, -1e-40), (0, 0, 1), (0, 0, -1), (0, 0, 0), (np.nan, 0, -1),
                       (1e-20, 0, -1e-30), (0.3, 0.1, -1)], F32)
    eo = np.resize(np.array([(0, 0, 2), (0.5, -0.5, 1e-7), (1, 1, -0.0), (0, 0, 1e20)], F32), (len(edge_d) ** 2, 3))
    ex, ey = np.meshgrid(np.arange(len(edge_d)), np.arange(len(edge_d)))
    return (np.concatenate([o, eo]), np.concatenate([dx, edge_d[ex.ravel()]]), np.concatenate([dy, edge_d[ey.ravel()]]))


def cases(blob, seed=0):
    rng = np.random.default_rng(seed)
    tex, maps, faces = tables(blob)
    uv = uv_grid(rng)
    out = [(0, 0, queries(a=uv))]
    for ti in range(len(tex)):
        out.append((1, ti, queries(a=uv)))
        # the filter: a sample of the uv set against every pair of edge differentials, plus random ones
        pick = uv[rng.choice(len(uv), 240, replace=False)]
        d0, d1 = np.meshgrid(np.arange(len(D_EDGES)), np.arange(len(D_EDGES)))
        de = np.array(D_EDGES, F32)
        ui = np.resize(np.arange(len(pick)), d0.size)
        out.append((2, ti, queries(a=pick[ui], b=de[d0.ravel()], c=de[d1.ravel()])))
        r = rng.uniform(-2, 2, (3000, 3)).astype(F32)
        scale = F32(10.0) ** rng.uniform(-6, 10, (3000, 1)).astype(F32)
        out.append((2, ti, queries(a=uv[rng.choice(len(uv), 3000)], b=(r * scale).astype(F32), c=(r[::-1] * scale).astype(F32))))
    colour = _f(0.9, 0.5, 0.25)
    for mi in list(range(len(maps))) + [-1]:
        out.append((3, mi, queries(a=uv, b=np.tile(colour, (len(uv), 1)))))
        sub = uv[rng.choice(len(uv), 600, replace=False)]
        de = np.array(D_EDGES, F32)
        di = rng.integers(0, len(de), (len(sub), 2))
        flag = np.resize(_f(1, 1, 1, 0), len(sub))
        out.append((4, mi, queries(a=sub, b=de[di[:, 0]], c=de[di[:, 1]], d=np.tile(colour, (len(sub), 1)), flag=flag)))
        dirs = _directions(rng, 2000)
        out.append((5, mi, queries(a=dirs, b=np.tile(colour, (len(dirs), 1)))))
    o, dx, dy = _diff_cases(rng, 3000)
    # plane: hit points on the unit plane (z = 0) and on its edges
    p = np.concatenate([rng.uniform(-1, 1, (len(o), 2)), np.zeros((len(o), 1))], axis=1).astype(F32)
    p[:8, :2] = [(1, 1), (-1, -1), (1, -1), (-1, 1), (0, 0), (-0.0, 1), (0.99999994, -0.99999994), (1e-45, -1e-45)]
    out.append((6, 0, queries(a=o, b=dx, c=dy, d=p)))
    # sphere: unit-sphere hits with N = p, and a tangent plane through the origin (p_x = 0: 1 / length(p_x) = inf)
    s = rng.normal(size=(len(o), 3))
    s = (s / np.linalg.norm(s, axis=1, keepdims=True)).astype(F32)
    n = s.copy()
    edge = queries(a=[(-1, 0, 0), (0, -2, 0)], b=[(1, 0, 0), (0, 1, 0)], c=[(1, 0, 0), (0, 1, 1e-30)], d=[(0, 0, 1), (0, 0, -1)],
                   e=[(1, 0, 0), (0, 1, 0)])
    out.append((7, 0, np.concatenate([queries(a=o * F32(3), b=dx, c=dy, d=s, e=n), edge])))
    # triangles of mesh 0 (index: mesh << 20 | element): barycentrics inside, on the edges and at the corners
    for el in range(faces):
        ab = rng.dirichlet((1, 1, 1), len(o))[:, :2].astype(F32)
        ab[:6] = [(1, 0), (0, 1), (0, 0), (0.5, 0.5), (1e-45, 1 - 2 ** -24), (0.3333333, 0.3333333)]
        out.append((8, el, queries(a=o, b=dx, c=dy, d=np.concatenate([ab, np.zeros((len(ab), 1), F32)], axis=1))))
    return out


def test_probe_scene_has_every_table_case(probe_blob):
    tex, maps, faces = tables(probe_blob)
    sizes = {(int(t["width"]), int(t["height"])) for t in tex if t["type"] == 1}
    assert set(TEX_SIZES) <= sizes and (tex["type"] == 0).any()
    assert (maps["texture"] == -1).any()
    assert np.isclose(np.abs(maps["itm"]).max(), 1e10, rtol=1e-6)
    assert faces == 5


def test_host_probe_equals_oracle_bit_for_bit(probe_blob):
    from oracle import binding as oracle
    total = 0
    for op, index, q in cases(probe_blob):
        h = host_probe(probe_blob, op, index, q)
        o = oracle.texture_probe(probe_blob, op, index, q)
        if not same_bits(h, o):
            bad = np.nonzero(~np.all((h.view(np.uint32) == o.view(np.uint32)) | (np.isnan(h) & np.isnan(o)), axis=1))[0]
            raise AssertionError(f"op {op} index {index}: {len(bad)} of {len(q)} differ, first input {q[bad[0]].tolist()}: "
                                 f"host {h[bad[0]].tolist()} oracle {o[bad[0]].tolist()}")
        total += len(q)
    assert total > 150000


def test_huge_uv_takes_the_x86_conversion():
    """The reference's (int) casts give INT_MIN from 2^31 on: uvw - (int) uvw is then uvw + 2^31, which tileClamp keeps."""
    x = _f(2147483520.0, 2 ** 31, 3e9, 1e10, -3e9, np.nan)
    out = host_probe(None, 0, 0, queries(a=np.stack([x, x, x], axis=1)))[:, 0]
    want = (x.astype(np.float64) - np.where(np.abs(x) < 2 ** 31, np.trunc(np.nan_to_num(x)), -2.0 ** 31)).astype(F32)
    want[x == 2147483520.0] = 0
    assert same_bits(out, want)
    assert same_bits(out[1:4], _f(4.2949673e9, 5.1474836e9, 1.2147484e10)) and out[4] < 0   # (-3e9 stays negative after += 1)


def test_conversion_helper_equals_x86_cast_strided(tmp_path):
    """qa_f2i_x86 (op 9) against cvttss2si over every 64th block of 65536 float bit patterns: both signs, every exponent, NaN and
    infinities (stride 1, every float, passes too: tests/cpp/texture_f2i.c)."""
    from qaray_amd import hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "texture_f2i")
    subprocess.run(["gcc", "-O2", "-fopenmp", os.path.join(root, "tests", "cpp", "texture_f2i.c"), "-o", exe, "-ldl"], check=True)
    r = subprocess.run([exe, hip.HIP_LIB_PATH, "64"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 mismatches" in r.stdout
    edges = _f(2147483520.0, 2 ** 31, -2 ** 31, np.nextafter(F32(-2 ** 31), F32(-np.inf)), 3e9, -3e9, np.inf, -np.inf, np.nan, -0.0, 0.99999994, -1.5)
    got = host_probe(None, 9, 0, queries(a=np.stack([edges] * 3, axis=1)))[:, 0].view(np.int32)
    assert got.tolist() == [2147483520, -2 ** 31, -2 ** 31, -2 ** 31, -2 ** 31, -2 ** 31, -2 ** 31, -2 ** 31, -2 ** 31, 0, 0, -1]
