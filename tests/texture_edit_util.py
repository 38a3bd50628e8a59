"""Shared by tests/test_texture_edit_host.py and tests/test_gpu_texture_edit.py: scene B = scene A after the edits the texture-edit
API can apply (qa_scene_edit_texels / texmaps / textures / backdrop), as a blob of its own (A's bytes patched in place) and as the
steps a context is given one call at a time."""
import numpy as np

QA_TEX_CHECKER, QA_TEX_FILE = 0, 1


def file_textures(blob):
    from qaray_amd import hip
    tex = hip.blob_table(blob, "textures")
    return [i for i in range(len(tex)) if tex[i]["type"] == QA_TEX_FILE and tex[i]["width"] > 0 and tex[i]["height"] > 0]


def paint(rng, h, w):
    """Random texels with both ends of the byte range among them."""
    px = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    px.reshape(-1)[0], px.reshape(-1)[-1] = 0, 255
    return px


def odd_rect(w, h):
    """A rectangle that starts at an odd column, is no multiple of 4 wide and leaves rows above and below, where the size allows."""
    x0 = 1 if w > 2 else 0
    x1 = max(x0 + 1, w - (2 if w > 4 else 0))
    if (x1 - x0) % 4 == 0 and x1 - x0 > 1:
        x1 -= 1
    y0 = h // 3
    y1 = max(y0 + 1, h - h // 4)
    return x0, y0, x1, y1


def make_b(blob_a, seed=5):
    """-> (blob B, steps): B is a patched copy of A; steps is a list of (kind, args...) in the order a context gets them:
    ('texels_host' | 'texels_device', texture, (x0, y0), rgb8), ('texmaps', first, records), ('textures', first, records),
    ('backdrop', background, environment).  Kinds a scene has nothing for are left out."""
    from qaray_amd import hip
    rng = np.random.default_rng(seed)
    b = np.array(blob_a, np.uint8, copy=True)
    steps = []
    tex = hip.blob_table(b, "textures")
    maps = hip.blob_table(b, "texmaps")
    files = sorted(file_textures(b), key=lambda i: -int(tex[i]["width"]) * int(tex[i]["height"]))
    if files:
        ti = files[0]
        w, h = int(tex[ti]["width"]), int(tex[ti]["height"])
        x0, y0, x1, y1 = odd_rect(w, h)
        px = paint(rng, y1 - y0, x1 - x0)
        hip.blob_texels(b, ti)[y0:y1, x0:x1] = px
        steps.append(("texels_host", ti, (x0, y0), px))
        # from device memory: the whole of another file texture, or the top rows of the same one
        tj = files[1] if len(files) > 1 else ti
        w, h = int(tex[tj]["width"]), int(tex[tj]["height"])
        rows = h if tj != ti else max(1, y0)
        px = paint(rng, rows, w)
        hip.blob_texels(b, tj)[:rows] = px
        steps.append(("texels_device", tj, (0, 0), px))
    shown = [k for k in range(len(maps)) if maps[k]["texture"] >= 0]
    if shown:
        k = shown[0]
        maps[k]["itm"] *= np.float32(1.25)
        maps[k]["pos"] += np.array([0.375, -0.125, 0.0], np.float32)
        steps.append(("texmaps", k, maps[k:k + 1].copy()))
        # a map that shows a file texture now shows another resident texture
        on_file = [k for k in shown if maps[k]["texture"] in files]
        if on_file and len(tex) > 1:
            k = on_file[-1]
            cur = int(maps[k]["texture"])
            others = [i for i in files if i != cur] or [i for i in range(len(tex)) if i != cur]
            maps[k]["texture"] = others[0]
            steps.append(("texmaps", k, maps[k:k + 1].copy()))
    checkers = [i for i in range(len(tex)) if tex[i]["type"] == QA_TEX_CHECKER]
    used = {int(m["texture"]) for m in maps}
    checkers = [i for i in checkers if i in used] or checkers
    if checkers:
        i = checkers[0]
        tex[i]["color1"] = np.array([0.875, 0.125, 0.25], np.float32)
        tex[i]["color2"] = tex[i]["color2"] * np.float32(0.5)
        steps.append(("textures", i, tex[i:i + 1].copy()))
    bg, env = hip.blob_backdrop(b)
    bg["color"] = np.array([0.25, 0.5, 0.125], np.float32)
    env["color"] = env["color"] * np.float32(0.5) + np.float32(0.125)
    steps.append(("backdrop", bg.copy(), env.copy()))
    return b, steps


def apply_step(ctx, step, device=None):
    """One step of make_b on a context; a 'texels_device' step goes through a torch tensor on `device` (default: the context's)."""
    kind = step[0]
    if kind == "texels_host":
        ctx.edit_texels(step[1], step[3], origin=step[2])
    elif kind == "texels_device":
        import torch
        t = torch.from_numpy(step[3]).to(device or torch.device("cuda", ctx.device_id))
        ctx.edit_texels(step[1], t, origin=step[2])
        return t   # (kept alive by the caller until the context has consumed it)
    elif kind == "texmaps":
        ctx.edit_texmaps(step[1], step[2])
    elif kind == "textures":
        ctx.edit_textures(step[1], step[2])
    else:
        ctx.edit_backdrop(step[1], step[2])
    return None


def apply_steps(ctx, steps):
    keep = [apply_step(ctx, s) for s in steps]
    ctx.synchronize()
    return keep
