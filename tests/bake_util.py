"""What the bake-map tests share (qa_bake.hip; the opening comment of qa_bake_dev.h is the specification): the float32 numpy restatement
of the map and of the gutter fill, the inside rule in rational arithmetic, a float64 restatement of a covered texel's point and normal,
and the scenes the tests write (XML + OBJ + PPM into a directory of the test's) with the blobs made of them.  Everything here reads the
mesh from the blob, as the library does: the loader may reorder an OBJ file's faces."""
import os
from fractions import Fraction

import numpy as np

F32 = np.float32
QA_OBJ_SPHERE, QA_OBJ_PLANE, QA_OBJ_MESH = 1, 2, 3
MAX_TILES = 4
EINVAL, EUNSUPPORTED = -1, -6


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def mesh_arrays(blob, mesh):
    """hip.blob_mesh_arrays: writable views of a mesh's faces, vertices, normals and texcoords"""
    from qaray_amd import hip
    return hip.blob_mesh_arrays(blob, mesh)


PLANE_XY = F32([[-1, -1], [1, -1], [1, 1], [-1, 1]])
PLANE_FACES = ((0, 1, 2), (0, 2, 3))


def node_faces(blob, node, mtl=-1):
    """The faces of a node as the map takes them -> list of (face id, uv (3, 2) f32 or None for a face without vt, V (3, 3) f32,
    N (3, 3) f32), the faces another mtl filters out left out"""
    from qaray_amd import hip
    inst = hip.blob_table(blob, "instances")[node]
    out = []
    if inst["obj_type"] == QA_OBJ_PLANE:
        if mtl >= 0 and mtl != 0:
            return out
        for f, corners in enumerate(PLANE_FACES):
            xy = PLANE_XY[list(corners)]
            uv = ((xy + F32(1)) * F32(0.5)).astype(F32)
            V = np.concatenate([xy, np.zeros((3, 1), F32)], axis=1)
            out.append((f, uv, V, np.tile(F32([0, 0, 1]), (3, 1))))
        return out
    assert inst["obj_type"] == QA_OBJ_MESH
    m = mesh_arrays(blob, int(inst["mesh"]))
    for f, fc in enumerate(m["faces"]):
        if mtl >= 0 and fc["mtl"] != mtl:
            continue
        vt = fc["vt"]
        uv = None if (vt < 0).any() or (vt >= len(m["texcoords"])).any() else m["texcoords"][vt].copy()
        out.append((f, uv, m["vertices"][fc["v"]].copy(), m["normals"][fc["vn"]].copy()))
    return out


def samples(W, H):
    """-> (sx (W,), sy (H,)) float32: the sample of texel (ix, iy) is (sx[ix], sy[iy])"""
    sx = (np.arange(W).astype(F32) / F32(W)).astype(F32)
    iy = np.arange(H).astype(F32)
    sy = np.where(np.arange(H) == 0, F32(0), (F32(1) - (iy / F32(H)).astype(F32)).astype(F32)).astype(F32)
    return sx, sy


def mul_mv(m, x, y, z):
    """mat3 (column-major, 9 floats) * (x, y, z), in glm's order, float32"""
    m = np.asarray(m, F32)
    return tuple(((m[r] * x + m[3 + r] * y).astype(F32) + m[6 + r] * z).astype(F32) for r in range(3))


def mul_tmv(m, x, y, z):
    m = np.asarray(m, F32)
    return tuple(((m[3 * c] * x + m[3 * c + 1] * y).astype(F32) + m[3 * c + 2] * z).astype(F32) for c in range(3))


def texture_vertices(blob, uv, texmap):
    """T (3, 2) float32 of a face's uv (3, 2) through texmap `texmap` (None: the raw uv)"""
    if texmap is None:
        return uv.astype(F32)
    from qaray_amd import hip
    rec = hip.blob_table(blob, "texmaps")[texmap]
    pos = rec["pos"].astype(F32)
    qx, qy, qz = (uv[:, 0] - pos[0]).astype(F32), (uv[:, 1] - pos[1]).astype(F32), np.full(3, F32(0) - pos[2], F32)
    tx, ty, _ = mul_mv(rec["itm"], qx, qy, qz)
    return np.stack([tx, ty], axis=1).astype(F32)


def face_setup(T):
    """The setup of a face from its T (3, 2) f32 -> None for a void face, else dict d, fm0, fn0, nm, nn, box (bx0, bx1, by0, by1);
    nm or nn above MAX_TILES is reported as they are"""
    if T is None or not np.isfinite(T).all():
        return None
    with np.errstate(over="ignore", invalid="ignore"):
        d = F32(F32(F32(T[1, 0] - T[0, 0]) * F32(T[2, 1] - T[0, 1])) - F32(F32(T[2, 0] - T[0, 0]) * F32(T[1, 1] - T[0, 1])))
    if d == 0 or not np.isfinite(d):
        return None
    bx0, bx1, by0, by1 = T[:, 0].min(), T[:, 0].max(), T[:, 1].min(), T[:, 1].max()
    fm0, fn0 = np.floor(bx0), np.floor(by0)
    cm, cn = F32(F32(np.floor(bx1) - fm0) + F32(1)), F32(F32(np.floor(by1) - fn0) + F32(1))
    return {"d": d, "fm0": F32(fm0), "fn0": F32(fn0), "cm": float(cm), "cn": float(cn), "box": (bx0, bx1, by0, by1)}


def over_tiles(blob, node, texmap=None, mtl=-1):
    for _, uv, _, _ in node_faces(blob, node, mtl):
        s = face_setup(None if uv is None else texture_vertices(blob, uv, texmap))
        if s and (not s["cm"] <= MAX_TILES or not s["cn"] <= MAX_TILES):
            return True
    return False


def root_identity(inst):
    r = inst[0]
    return (r["tm"].tobytes() == np.eye(3, dtype=F32).tobytes() and r["itm"].tobytes() == np.eye(3, dtype=F32).tobytes()
            and r["pos"].tobytes() == np.zeros(3, F32).tobytes())


def bake_ref(blob, node, W, H, texmap=None, mtl=-1):
    """The specification in float32 numpy, every operation rounded as written -> dict point, normal, face, bary"""
    from qaray_amd import hip
    inst = hip.blob_table(blob, "instances")
    sx, sy = samples(W, H)
    SX, SY = np.broadcast_to(sx[None, :], (H, W)), np.broadcast_to(sy[:, None], (H, W))
    face = np.full((H, W), -1, np.int32)
    E0, E1, D = np.zeros((H, W), F32), np.zeros((H, W), F32), np.ones((H, W), F32)
    VV, NN = np.zeros((H, W, 3, 3), F32), np.zeros((H, W, 3, 3), F32)
    with np.errstate(all="ignore"):
        for f, uv, V, N in node_faces(blob, node, mtl):
            T = None if uv is None else texture_vertices(blob, uv, texmap)
            s = face_setup(T)
            if s is None:
                continue
            assert s["cm"] <= MAX_TILES and s["cn"] <= MAX_TILES
            bx0, bx1, by0, by1 = s["box"]
            for i in range(int(s["cn"])):
                for j in range(int(s["cm"])):
                    px = (SX + F32(s["fm0"] + F32(j))).astype(F32)
                    py = (SY + F32(s["fn0"] + F32(i))).astype(F32)
                    box = (px >= bx0) & (px <= bx1) & (py >= by0) & (py <= by1)
                    x = [(T[q, 0] - px).astype(F32) for q in range(3)]
                    y = [(T[q, 1] - py).astype(F32) for q in range(3)]
                    e0 = ((x[1] * y[2]).astype(F32) - (x[2] * y[1]).astype(F32)).astype(F32)
                    e1 = ((x[2] * y[0]).astype(F32) - (x[0] * y[2]).astype(F32)).astype(F32)
                    e2 = ((x[0] * y[1]).astype(F32) - (x[1] * y[0]).astype(F32)).astype(F32)
                    if s["d"] < 0:
                        e0, e1, e2 = -e0, -e1, -e2
                    new = box & (e0 >= 0) & (e1 >= 0) & (e2 >= 0) & (face < 0)
                    face[new] = f
                    E0[new], E1[new], D[new] = e0[new], e1[new], s["d"]
                    VV[new], NN[new] = V, N
        cov = face >= 0
        ad = np.abs(D)
        a, b = (E0 / ad).astype(F32), (E1 / ad).astype(F32)
        c = ((F32(1) - a).astype(F32) - b).astype(F32)

        def mix(X):   # (X0 * a + X1 * b) + X2 * c, per component
            return [((X[..., 0, k] * a).astype(F32) + (X[..., 1, k] * b).astype(F32)).astype(F32) + (X[..., 2, k] * c).astype(F32) for k in range(3)]
        p, n = [v.astype(F32) for v in mix(VV)], [v.astype(F32) for v in mix(NN)]

        def normalize(v):
            dot = (((v[0] * v[0]).astype(F32) + (v[1] * v[1]).astype(F32)).astype(F32) + (v[2] * v[2]).astype(F32)).astype(F32)
            r = (F32(1) / np.sqrt(dot)).astype(F32)
            return [(k * r).astype(F32) for k in v]
        at = int(node)
        ident = root_identity(inst)
        while at >= 0:
            if at == 0 and ident:
                n = normalize(n)
                break
            rec = inst[at]
            q = mul_mv(rec["tm"], *p)
            p = [(q[k] + rec["pos"][k]).astype(F32) for k in range(3)]
            n = normalize(list(mul_tmv(rec["itm"], *n)))
            at = int(rec["parent"])
    out = {"point": np.stack(p, axis=2), "normal": np.stack(n, axis=2), "face": face, "bary": np.stack([a, b], axis=2)}
    for k in ("point", "normal", "bary"):
        out[k] = np.where(cov[..., None], out[k], F32(0)).astype(F32)
    return out


def exact_faces(blob, node, W, H, texmap=None, mtl=-1):
    """The inside rule in rational arithmetic on the float32 T and the float32 samples (tiles as exact integers) -> (lowest, int32
    [H, W]: the lowest face that holds the sample, -1 for none; margin [H, W] float: the smallest |edge function| of the sample over
    the faces whose box holds it, in edge-function units: what tells a sample near an edge from one well inside or outside)"""
    sx, sy = samples(W, H)
    fx, fy = [Fraction(float(v)) for v in sx], [Fraction(float(v)) for v in sy]
    lowest = np.full((H, W), -1, np.int32)
    margin = np.full((H, W), np.inf)
    faces = []
    for f, uv, _, _ in node_faces(blob, node, mtl):
        T = None if uv is None else texture_vertices(blob, uv, texmap)
        if face_setup(T) is None:
            continue
        t = [(Fraction(float(T[q, 0])), Fraction(float(T[q, 1]))) for q in range(3)]
        d = (t[1][0] - t[0][0]) * (t[2][1] - t[0][1]) - (t[2][0] - t[0][0]) * (t[1][1] - t[0][1])
        if d == 0:
            continue   # (exactly degenerate although fp32 says otherwise: cannot hold a sample with all three >= 0 ... unless on it; left out)
        xs, ys = [q[0] for q in t], [q[1] for q in t]
        faces.append((f, t, 1 if d > 0 else -1, min(xs), max(xs), min(ys), max(ys)))
    for iy in range(H):
        for ix in range(W):
            for f, t, sign, x0, x1, y0, y1 in faces:
                hit = False
                for n in range(int(np.floor(float(y0))), int(np.floor(float(y1))) + 1):
                    py = fy[iy] + n
                    if py < y0 or py > y1:
                        continue
                    for m in range(int(np.floor(float(x0))), int(np.floor(float(x1))) + 1):
                        px = fx[ix] + m
                        if px < x0 or px > x1:
                            continue
                        e = [sign * ((t[(q + 1) % 3][0] - px) * (t[(q + 2) % 3][1] - py) - (t[(q + 2) % 3][0] - px) * (t[(q + 1) % 3][1] - py)) for q in range(3)]
                        margin[iy, ix] = min(margin[iy, ix], *(abs(float(v)) for v in e))
                        if min(e) >= 0:
                            hit = True
                if hit and lowest[iy, ix] < 0:
                    lowest[iy, ix] = f
    return lowest, margin


def point_normal_f64(blob, node, face, bary):
    """A covered texel's point and normal in float64 from its face and (a, b): forward interpolation and the node chain -> (point,
    normal, scale): scale is the largest magnitude met on the way per texel (what a tolerance in ulps is taken of)"""
    from qaray_amd import hip
    inst = hip.blob_table(blob, "instances")
    by_id = {f: (V.astype(np.float64), N.astype(np.float64)) for f, _, V, N in node_faces(blob, node)}
    H, W = face.shape
    P, Nn, S = np.zeros((H, W, 3)), np.zeros((H, W, 3)), np.zeros((H, W))
    for iy in range(H):
        for ix in range(W):
            f = int(face[iy, ix])
            if f < 0:
                continue
            V, N = by_id[f]
            a, b = float(bary[iy, ix, 0]), float(bary[iy, ix, 1])
            w = np.array([a, b, 1.0 - a - b])
            p, n = w @ V, w @ N
            scale = np.abs(w[:, None] * V).max()
            at = int(node)
            ident = root_identity(inst)
            while at >= 0:
                if at == 0 and ident:
                    break
                rec = inst[at]
                tm, itm = rec["tm"].astype(np.float64).reshape(3, 3).T, rec["itm"].astype(np.float64).reshape(3, 3).T
                scale = max(scale, np.abs(tm * p[None, :]).max(), np.abs(rec["pos"]).max())
                p = tm @ p + rec["pos"].astype(np.float64)
                n = itm.T @ n
                n = n / np.linalg.norm(n)
                at = int(rec["parent"])
            P[iy, ix], Nn[iy, ix], S[iy, ix] = p, n / np.linalg.norm(n), scale
    return P, Nn, S


def dilate_ref(rgb8, face, radius):
    """The gutter fill restated: plain loops over the candidates in the tie order"""
    H, W = face.shape
    out = rgb8.copy()
    cov = face >= 0
    order = sorted(((dx * dx + dy * dy, dy, dx) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1)))
    for y in range(H):
        for x in range(W):
            if cov[y, x]:
                continue
            for _, dy, dx in order:
                yy, xx = (y + dy) % H, (x + dx) % W
                if cov[yy, xx]:
                    out[y, x] = rgb8[yy, xx]
                    break
    return out


# ---- scenes ---------------------------------------------------------------------------------------

def obj_text(vertices, texcoords, normals, faces, mtllib=None):
    """An OBJ file: faces are lists of (v, vt, vn) 0-based triples (vt None: no texture vertex), or ("usemtl", name)"""
    lines = [f"mtllib {mtllib}"] if mtllib else []
    lines += ["v %.9g %.9g %.9g" % tuple(v) for v in vertices]
    lines += ["vt %.9g %.9g" % tuple(t) for t in texcoords]
    lines += ["vn %.9g %.9g %.9g" % tuple(n) for n in normals]
    for f in faces:
        if f[0] == "usemtl":
            lines.append(f"usemtl {f[1]}")
        else:
            lines.append("f " + " ".join(f"{v + 1}/{'' if vt is None else vt + 1}/{vn + 1}" for v, vt, vn in f))
    return "\n".join(lines) + "\n"


CAMERA = """<camera><position x="0" y="-14" z="6"/><target x="0" y="0" z="0.5"/><up x="0" y="0" z="1"/><fov value="40"/>
  <width value="48"/><height value="36"/></camera>"""
MATTE = """<material type="blinn" name="m"><diffuse r="0.7" g="0.6" b="0.5"/></material>"""
LAMP = """<light type="point" name="l"><intensity value="40"/><position x="3" y="-8" z="9"/></light>"""


def write_scene(root, objects, files=None, extra=MATTE + LAMP, size=(48, 36)):
    """Writes <root>/scene.xml around `objects` (XML text) and `files` (name -> text or bytes) -> the scene's blob"""
    from qaray_amd.host import load_scene_blob
    os.makedirs(root, exist_ok=True)
    for name, body in (files or {}).items():
        with open(os.path.join(root, name), "wb" if isinstance(body, bytes) else "w") as f:
            f.write(body)
    path = os.path.join(root, "scene.xml")
    with open(path, "w") as f:
        f.write(f"<xml><scene>\n{objects}\n{extra}\n</scene>{CAMERA}</xml>\n")
    return load_scene_blob(path, size=size, asset_root=str(root))


def ppm_bytes(rgb8):
    h, w = rgb8.shape[:2]
    return b"P6\n%d %d\n255\n" % (w, h) + np.ascontiguousarray(rgb8, np.uint8).tobytes()


def mesh_node(name, inner="", material="m"):
    return f'<object type="obj" name="{name}" material="{material}">{inner}</object>'


UP = [(0.0, 0.0, 1.0)]


def atlas_obj(no_vt_face=True):
    """The dyadic atlas: uv vertices on multiples of 1/64.  Chart A (faces 0, 1) a square split along a diagonal that passes through
    texel samples; chart B (faces 2, 3) with reversed winding; face 4 overlaps both; face 5 has zero uv area; face 6 has no vt (or,
    where a scene must upload, repeats face 5's)"""
    g = 1.0 / 64.0
    vt = [(4 * g, 4 * g), (28 * g, 4 * g), (28 * g, 28 * g), (4 * g, 28 * g),            # chart A
          (34 * g, 8 * g), (60 * g, 8 * g), (60 * g, 56 * g), (34 * g, 56 * g),          # chart B
          (16 * g, 16 * g), (48 * g, 20 * g), (30 * g, 50 * g),                           # the overlapping face
          (8 * g, 40 * g), (16 * g, 48 * g), (24 * g, 56 * g)]                            # collinear: zero area
    v = [(4 * u - 2, 4 * w - 2, 0.25 * k) for k, (u, w) in enumerate(vt)]
    tri = lambda *ids: [(i, i, 0) for i in ids]   # noqa: E731
    faces = [tri(0, 1, 2), tri(0, 2, 3), tri(4, 6, 5), tri(4, 7, 6), tri(8, 9, 10), tri(11, 12, 13)]
    faces.append([(11, None, 0), (12, None, 0), (13, None, 0)] if no_vt_face else tri(11, 12, 13))
    return obj_text(v, vt, UP, faces)


def grid_obj(nx, ny, seed=None, u0=0.0, u1=1.0, v0=0.0, v1=1.0, height=None):
    """A chart of nx x ny cells (two faces each) over [u0, u1] x [v0, v1]; seed: interior vertices jittered by up to 0.3 of a cell;
    the surface is z = height(u, v) (default: flat) with its own normals"""
    rng = np.random.default_rng(seed) if seed is not None else None
    vt, v, vn = [], [], []
    for j in range(ny + 1):
        for i in range(nx + 1):
            u, w = i / nx, j / ny
            if rng is not None and 0 < i < nx and 0 < j < ny:
                u += rng.uniform(-0.3, 0.3) / nx
                w += rng.uniform(-0.3, 0.3) / ny
            vt.append((u0 + (u1 - u0) * u, v0 + (v1 - v0) * w))
            z = height(u, w) if height else 0.0
            v.append((4 * u - 2, 4 * w - 2, z))
            if height:
                e = 1e-4
                n = np.array([-(height(u + e, w) - height(u - e, w)) / (8 * e), -(height(u, w + e) - height(u, w - e)) / (8 * e), 1.0])
                vn.append(tuple(n / np.linalg.norm(n)))
            else:
                vn.append((0.0, 0.0, 1.0))
    at = lambda i, j: j * (nx + 1) + i   # noqa: E731
    faces = []
    for j in range(ny):
        for i in range(nx):
            a, b, c, d = at(i, j), at(i + 1, j), at(i + 1, j + 1), at(i, j + 1)
            faces.append([(k, k, k) for k in (a, b, c)])
            faces.append([(k, k, k) for k in (a, c, d)])
    return obj_text(v, vt, vn, faces)


def dome(u, w):
    """A convex cap over the unit square of (u, w)"""
    return 1.5 - 1.2 * ((u - 0.5) ** 2 + (w - 0.5) ** 2)


TWO_MTL = "newmtl red\nKd 1 0 0\nnewmtl blue\nKd 0 0 1\n"


def two_material_obj():
    g = grid_obj(2, 2).splitlines()
    faces = [l for l in g if l.startswith("f ")]
    rest = [l for l in g if not l.startswith("f ")]
    return "\n".join(["mtllib two.mtl"] + rest + ["usemtl red"] + faces[:4] + ["usemtl blue"] + faces[4:]) + "\n"


NESTED = ('<object type="obj" name="outer.obj" material="m"><scale x="1.5" y="0.75" z="1.25"/><rotate angle="25" x="1" y="0.4" z="0.2"/>'
          '<translate x="0.5" y="1" z="2"/>%s</object>')
INNER = '<scale x="0.6" y="1.4" z="0.9"/><rotate angle="-40" x="0.2" y="1" z="0.3"/><translate x="-1" y="0.5" z="1.5"/>'


# ---- tolerances ------------------------------------------------------------------------------------
EPS = 2.0 ** -24   # half an ulp of a float32 in [1, 2): the relative error of one rounded operation


def point_tolerance(scale, levels):
    """The fp32 point against its float64 restatement from the same (a, b).  The interpolation is 3 products and 2 sums, c = 1 - a - b
    two more; a level of the chain 9 products and 8 sums into 3 components, 5 + 1 roundings on the path of one component.  Every
    rounding is at most EPS of the largest term it can meet (`scale`, taken by point_normal_f64 over every product and translation on the
    way), and a later level multiplies what came before by its matrix, whose rows sum to less than 4 for the nodes used here: so
    (7 + 6 * levels) roundings, each weighed by at most 4 ** levels.  -> absolute tolerance"""
    return (7 + 6 * levels) * 4.0 ** levels * EPS * scale


def normal_tolerance(levels, stretch):
    """The unit normal likewise: 7 roundings of the interpolation, then per level 5 for a component of mulTMV and 7 for the
    normalisation (dot: 5, sqrt, reciprocal, product: relative EPS each of a quantity near 1 after the division), each of which the
    next normalisation can stretch by at most `stretch` = the largest ratio of a node's itm singular values -> absolute tolerance on
    a component of a unit vector"""
    return (7 + 12 * max(levels, 1)) * stretch ** max(levels, 1) * EPS


def chain_levels(blob, node):
    from qaray_amd import hip
    inst = hip.blob_table(blob, "instances")
    ident = root_identity(inst)
    n, at = 0, int(node)
    while at >= 0 and not (at == 0 and ident):
        n += 1
        at = int(inst[at]["parent"])
    return n


def chain_stretch(blob, node):
    from qaray_amd import hip
    inst = hip.blob_table(blob, "instances")
    s, at = 1.0, int(node)
    while at > 0:
        sv = np.linalg.svd(inst[at]["itm"].astype(np.float64).reshape(3, 3), compute_uv=False)
        s = max(s, sv.max() / sv.min())
        at = int(inst[at]["parent"])
    return s


# ---- the cases every side runs ---------------------------------------------------------------------

def tri3_obj():
    vt = [(0.1, 0.1), (0.9, 0.15), (0.5, 0.5), (0.85, 0.9), (0.12, 0.8)]
    v = [(4 * u - 2, 4 * w - 2, 0.0) for u, w in vt]
    tri = lambda *ids: [(i, i, 0) for i in ids]   # noqa: E731
    return obj_text(v, vt, UP, [tri(0, 1, 2), tri(2, 1, 3), tri(0, 2, 4)])


def span_obj(tiles):
    """One face whose uv spans `tiles` tiles in u"""
    vt = [(0.25, 0.25), (tiles - 0.5, 0.25), (0.25, 0.75)]
    v = [(u, w, 0.0) for u, w in vt]
    return obj_text(v, vt, UP, [[(i, i, 0) for i in (0, 1, 2)]])


TEXTURED = ('<material type="blinn" name="t"><diffuse r="0" g="0" b="0"/><emission value="1" texture="ramp.ppm">'
            '<scale x="0.5" y="2"/><rotate angle="90" z="1"/><translate x="0.25" y="-0.5"/></emission></material>')


CHECKED = ('<material type="blinn" name="c"><diffuse r="1" g="1" b="1" texture="checkerboard"><color1 r="0.2" g="0.2" b="0.2"/>'
           '<color2 r="0.8" g="0.8" b="0.8"/><scale value="1.25"/><translate x="-0.125" y="-0.125"/></diffuse></material>')


def ramp_texels(w=32, h=16):
    """Texel (ix, iy) = (8 * ix, 16 * iy, 0)"""
    t = np.zeros((h, w, 3), np.uint8)
    t[..., 0] = 8 * np.arange(w)[None, :]
    t[..., 1] = 16 * np.arange(h)[:, None]
    return t


def emission_texmap(blob, material=0):
    from qaray_amd import hip
    return int(hip.blob_table(blob, "materials")[material]["emission"]["texmap"])


def build_cases(root, uploadable=False):
    """name -> dict blob, node, texmap (None or index), mtl, sizes.  uploadable: the variants a context accepts (an upload refuses a mesh
    with texture vertices on some faces only, so the atlas's face without vt repeats the void face instead)"""
    from qaray_amd import hip
    root = str(root)
    c = {}

    def add(name, objects, files, node=1, texmap=None, mtl=-1, sizes=((19, 13),), extra=MATTE + LAMP):
        blob = write_scene(os.path.join(root, name), objects, files, extra=extra)
        c[name] = {"blob": blob, "node": node, "texmap": texmap, "mtl": mtl, "sizes": sizes}
        return c[name]
    add("atlas", mesh_node("atlas.obj"), {"atlas.obj": atlas_obj(not uploadable)}, sizes=((32, 32), (16, 64)))
    add("chart", mesh_node("chart.obj"), {"chart.obj": grid_obj(6, 5, seed=7)}, sizes=((19, 13), (64, 64), (1, 1), (16, 16), (17, 16)))
    add("grid264", mesh_node("g.obj", '<rotate angle="30" z="1"/><translate z="1"/>'), {"g.obj": grid_obj(12, 11, height=dome)}, sizes=((17, 16), (64, 64)))
    add("tri3", mesh_node("t.obj"), {"t.obj": tri3_obj()})
    add("nested", NESTED % mesh_node("dome.obj", INNER), {"outer.obj": tri3_obj(), "dome.obj": grid_obj(4, 4, height=dome)}, node=2)
    add("tile_up", mesh_node("g.obj"), {"g.obj": grid_obj(3, 3, seed=3, u0=1.25, u1=1.75, v0=1.25, v1=1.75)})
    add("tile_negative", mesh_node("g.obj"), {"g.obj": grid_obj(3, 3, seed=4, u0=-0.75, u1=-0.25, v0=-1.5, v1=-1.0)})
    add("straddle", mesh_node("g.obj"), {"g.obj": grid_obj(3, 2, seed=5, u0=0.5, u1=2.5, v0=-0.25, v1=0.5)})
    t = add("texmap", mesh_node("g.obj", material="t"), {"g.obj": grid_obj(3, 3, seed=6, u0=0.05, u1=0.95, v0=0.05, v1=0.95, height=dome), "ramp.ppm": ppm_bytes(ramp_texels())},
            sizes=((32, 16), (19, 13)), extra=TEXTURED)   # (no light: what a ray sees of it is its emission)
    t["texmap"] = emission_texmap(t["blob"])
    # the convex cap and the plane with their charts kept off the border of the texture, so that no covered sample lies on the
    # surface's own border (where a ray cast at it may pass by)
    add("convex", mesh_node("g.obj", '<scale x="1.5" y="1" z="1"/><rotate angle="30" z="1"/><translate x="0.5" z="1"/>'),
        {"g.obj": grid_obj(6, 5, seed=8, u0=0.03, u1=0.97, v0=0.04, v1=0.96, height=dome)}, sizes=((19, 13), (48, 40)))
    p = add("plane_inset", '<object type="plane" name="p" material="c"><scale x="3" y="2" z="1"/><rotate angle="20" x="1" y="0.2"/><translate z="0.5"/></object>',
            None, sizes=((19, 13), (16, 16)), extra=CHECKED + LAMP)
    p["texmap"] = int(hip.blob_table(p["blob"], "materials")[0]["diffuse"]["texmap"])
    for mtl in (-1, 0, 1):
        add(f"two_mtl_{mtl}", mesh_node("two.obj"), {"two.obj": two_material_obj(), "two.mtl": TWO_MTL}, mtl=mtl)
    add("plane", '<object type="plane" name="p" material="m"><scale x="3" y="2" z="1"/><rotate angle="20" x="1" y="0.2"/><translate z="0.5"/></object>', None,
        sizes=((16, 16), (19, 13)))
    return c
