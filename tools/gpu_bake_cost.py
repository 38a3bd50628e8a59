#!/usr/bin/env python3
"""What a bake map costs: on the cube of custom_textures.xml (12 faces) and on the first textured mesh of bench.py's C3
frame (example_project7_object.xml, 27 794 faces), at 256 x 256 and 1024 x 1024 texels, raw uv (no texmap).  Per configuration the calls
take turns inside every repeat, each between two events on the caller's stream, same library, same stream:
  bake_texels   Context.bake_texels_device, the four planes (36 bytes written per texel)
  bake_dilate   Context.bake_dilate_device at radius 2 over a random picture and a face plane with gutters: the map's, with the texels
                outside 8 x 8 blocks on a 12-texel grid marked uncovered (56 % of them, every one within the radius of a block), so
                that the gather runs - raw uv wraps these meshes over the whole texture and leaves no gutter of its own
  ao_points     the Context.ao_points_device call that follows in bake_ao, at K = 16, radius unbounded, over every texel's point
  torch         the same map as a user would write it today: the inside rule as one broadcast texels x faces expression in torch, the
                first inside face by argmax, weights and point by gathers, in strips of rows of at most 2^24 texel-face pairs.  One
                tile only and no node transform: the row is a cost, its planes are not compared
After warm-up rounds, the medians of --repeats rounds.  Nothing is fixed in advance: the rows are the measurement, with the ratio
bake_texels / torch.  Each configuration runs in a child process of its own under a time limit (--limit seconds), by the rule of
tools/cost.py.  Needs a GPU: there is no fallback."""
import sys

import numpy as np

import cost

TOOL = "gpu_bake_cost"
CONFIGS = {"cube": "custom_textures.xml", "c3": "example_project7_object.xml"}
SIZES = (256, 1024)
K = 16
STRIP_PAIRS = 1 << 24


def textured_mesh(hip, blob):
    """-> (node, faces' uv (F, 3, 2), faces' vertices (F, 3, 3)) of the first mesh node with texture vertices"""
    inst, meshes = hip.blob_table(blob, "instances"), hip.blob_table(blob, "meshes")
    for node, rec in enumerate(inst):
        if rec["obj_type"] == 3 and meshes[rec["mesh"]]["num_texcoords"] > 0:
            m = hip.blob_mesh_arrays(blob, int(rec["mesh"]))
            return node, m["texcoords"][m["faces"]["vt"]].copy(), m["vertices"][m["faces"]["v"]].copy()
    raise SystemExit(f"{TOOL}: no mesh with texture vertices in the scene")


def torch_map(torch, T, V, W, H, out_face, out_bary, out_point):
    """The broadcast expression, strip by strip, on the current stream"""
    F = T.shape[0]
    d = (T[:, 1, 0] - T[:, 0, 0]) * (T[:, 2, 1] - T[:, 0, 1]) - (T[:, 2, 0] - T[:, 0, 0]) * (T[:, 1, 1] - T[:, 0, 1])
    sign = torch.sign(d)
    sx = torch.arange(W, device=T.device, dtype=torch.float32) / W
    rows = max(1, STRIP_PAIRS // (W * F))
    for y in range(0, H, rows):
        y1 = min(H, y + rows)
        iy = torch.arange(y, y1, device=T.device, dtype=torch.float32)
        sy = torch.where(iy == 0, torch.zeros_like(iy), 1 - iy / H)
        px = sx.repeat(y1 - y)[:, None]
        py = sy.repeat_interleave(W)[:, None]
        x0, y0, x1, y1_, x2, y2 = T[:, 0, 0] - px, T[:, 0, 1] - py, T[:, 1, 0] - px, T[:, 1, 1] - py, T[:, 2, 0] - px, T[:, 2, 1] - py
        e0, e1, e2 = (x1 * y2 - x2 * y1_) * sign, (x2 * y0 - x0 * y2) * sign, (x0 * y1_ - x1 * y0) * sign
        inside = (e0 >= 0) & (e1 >= 0) & (e2 >= 0) & (d != 0)
        first = inside.to(torch.int8).argmax(dim=1)
        any_ = inside.any(dim=1)
        a = e0.gather(1, first[:, None])[:, 0] / d.abs()[first]
        b = e1.gather(1, first[:, None])[:, 0] / d.abs()[first]
        c = 1 - a - b
        p = V[first, 0] * a[:, None] + V[first, 1] * b[:, None] + V[first, 2] * c[:, None]
        lo, hi = y * W, y1 * W
        out_face.view(-1)[lo:hi] = torch.where(any_, first.to(torch.int32), torch.full_like(first, -1, dtype=torch.int32))
        out_bary.view(-1, 2)[lo:hi] = torch.stack([a, b], dim=1) * any_[:, None]
        out_point.view(-1, 3)[lo:hi] = p * any_[:, None]


def measure(tag, warmup, repeats):
    torch, hip = cost.gpu(TOOL)
    cost.assets()
    ctx, blob, _, dev, s = cost.open_scene(TOOL, (CONFIGS[tag], 256, 192))
    node, uv, verts = textured_mesh(hip, blob)
    T, V = torch.from_numpy(uv).to(dev), torch.from_numpy(verts).to(dev)
    for size in SIZES:
        W = H = size
        planes = ctx.bake_texels_device(node, W, H, stream=s.cuda_stream)
        s.synchronize()
        covered = float((planes["face"] >= 0).float().mean())
        grey = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device=dev)
        filled = torch.empty_like(grey)
        k = torch.arange(size, device=dev) % 12 < 8
        gutters = torch.where(k[:, None] & k[None, :], planes["face"], torch.full_like(planes["face"], -1))
        uncovered = float((gutters < 0).float().mean())
        ids = torch.arange(W * H, dtype=torch.int32, device=dev)
        ao = {"open": torch.empty(W * H, dtype=torch.int32, device=dev), "ao": torch.empty(W * H, dtype=torch.float32, device=dev)}
        tf, tb, tp = torch.empty((H, W), dtype=torch.int32, device=dev), torch.empty((H, W, 2), device=dev), torch.empty((H, W, 3), device=dev)
        points, normals = planes["point"].reshape(-1, 3), planes["normal"].reshape(-1, 3)

        def torch_row():
            with torch.cuda.stream(s):
                torch_map(torch, T, V, W, H, tf, tb, tp)
        calls = {"bake_texels": lambda: ctx.bake_texels_device(node, W, H, stream=s.cuda_stream, **planes),
                 "bake_dilate": lambda: ctx.bake_dilate_device(grey, gutters, 2, out=filled, stream=s.cuda_stream),
                 "ao_points": lambda: ctx.ao_points_device(points, normals, K, stream_ids=ids, stream=s.cuda_stream, **ao),
                 "torch": torch_row}
        spans = cost.timed_turns(s, calls, list(calls), warmup, repeats)
        bake = cost.summary(spans["bake_texels"])
        for name, t in spans.items():
            row = cost.summary(t)
            more = {"bake_texels_over_this": round(bake["median_ms"] / row["median_ms"], 4)} if name == "torch" else {}
            if name == "bake_dilate":
                more = {"uncovered": round(uncovered, 4)}
            cost.emit(TOOL, f"{tag} {size} {name}", config=tag, scene=CONFIGS[tag], node=node, faces=int(T.shape[0]), texels=[W, H], covered=round(covered, 4),
                      what=name, **row, **more)
    ctx.close()


def main():
    ap = cost.arguments(__doc__, one=tuple(CONFIGS))
    a = ap.parse_args()
    if a.one:
        return measure(a.one, a.warmup, a.repeats)
    cost.run_children(__file__, [[tag] for tag in CONFIGS], sys.argv[1:], a.limit)


if __name__ == "__main__":
    main()
