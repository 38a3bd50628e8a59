"""Shared by tests/test_scene_edit_host.py and tests/test_gpu_scene_edit.py: scene B = scene A after the edits the scene-edit
API can apply (qa_scene_edit_*), made two ways - as a blob of its own (the XML with a rewritten <camera>, flattened, then the
light / material / node records patched in the blob) and as the records a context is given one edit at a time."""
import os
import re
import xml.etree.ElementTree as ET

import numpy as np

QA_LIGHT_AMBIENT, QA_LIGHT_DIRECT, QA_LIGHT_POINT, QA_LIGHT_SPOT = 0, 1, 2, 3


def scene_path(name):
    from qaray_amd.host import SCENES_DIR
    return os.path.join(SCENES_DIR, name)


def xml_camera(path):
    """The <camera> of a scene file -> dict(pos, target, up, fov, focaldist, dof) with the loader's defaults."""
    cam = ET.parse(path).getroot().find("camera")
    out = {"pos": [0.0, 0.0, 0.0], "target": [0.0, 0.0, -1.0], "up": [0.0, 1.0, 0.0], "fov": 40.0, "focaldist": 1.0, "dof": 0.0}
    for e in cam:
        if e.tag in ("position", "target", "up"):
            key = "pos" if e.tag == "position" else e.tag
            out[key] = [float(e.get(a, out[key][i])) for i, a in enumerate("xyz")]
        elif e.tag in ("fov", "focaldist", "dof"):
            out[e.tag] = float(e.get("value"))
    return out


def moved_camera(cam):
    """Another view of the same scene: the eye a twelfth of the way round the target and a little up, a narrower lens; every number
    a float32 that prints exactly, so that the XML text and the setter's arguments are the same floats."""
    f32 = lambda v: [float(np.float32(x)) for x in v]   # noqa: E731
    pos, target = np.array(cam["pos"], np.float64), np.array(cam["target"], np.float64)
    d = pos - target
    up = np.array(cam["up"], np.float64)
    side = np.cross(up, d)
    new = target + 0.96 * d + 0.25 * side + 0.06 * np.linalg.norm(d) * up / max(np.linalg.norm(up), 1e-9)
    out = dict(cam)
    out["pos"] = f32(new)
    out["target"] = f32(target + 0.02 * side)
    out["fov"] = float(np.float32(cam["fov"] * 0.9))
    if cam["dof"] > 0:
        out["dof"] = float(np.float32(cam["dof"] * 1.5))
        out["focaldist"] = float(np.float32(cam["focaldist"] * 0.95))
    return out


def write_xml_with_camera(src, dst, cam, size):
    """A copy of scene file `src` whose <camera> element is rewritten to `cam` (and the image size)."""
    text = open(src).read()
    v = lambda tag, p: '<%s x="%s" y="%s" z="%s"/>' % ((tag,) + tuple(repr(float(x)) for x in p))   # noqa: E731
    block = "<camera>\n    %s\n    %s\n    %s\n" % (v("position", cam["pos"]), v("target", cam["target"]), v("up", cam["up"]))
    block += '    <fov value="%r"/>\n    <focaldist value="%r"/>\n    <dof value="%r"/>\n' % (cam["fov"], cam["focaldist"], cam["dof"])
    block += '    <width value="%d"/>\n    <height value="%d"/>\n  </camera>' % size
    new, n = re.subn(r"<camera>.*?</camera>", lambda m: block, text, flags=re.S)
    assert n == 1
    with open(dst, "w") as f:
        f.write(new)


def host_scene(name, size):
    from qaray_amd.host import HostScene
    return HostScene(scene_path(name), size=size)


def rotation(deg, axis):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return (np.eye(3) * c + s * K + (1 - c) * np.outer(a, a)).astype(np.float32)


def patch_records(blob):
    """Edits one light (moved and dimmed), one material (diffuse and reflection colours) and one node (translated and rotated) in
    `blob` in place -> {'lights': (first, records), 'materials': ..., 'instances': ...}: the records to hand a context."""
    from qaray_amd import hip
    out = {}
    lights = hip.blob_table(blob, "lights")
    cand = [i for i in range(len(lights)) if lights[i]["type"] in (QA_LIGHT_POINT, QA_LIGHT_SPOT)] or \
           [i for i in range(len(lights)) if lights[i]["type"] != QA_LIGHT_AMBIENT]
    if cand:
        i = cand[0]
        lights[i]["position"] += np.array([0.5, -0.25, 0.375], np.float32)
        d = lights[i]["direction"] + np.array([0.125, 0.0, -0.0625], np.float32)
        if lights[i]["type"] != QA_LIGHT_POINT:
            lights[i]["direction"] = d / np.float32(np.sqrt(np.float32(d @ d)))
        lights[i]["intensity"] *= np.float32(0.75)
        out["lights"] = (i, lights[i:i + 1].copy())
    mats = hip.blob_table(blob, "materials")
    if len(mats):
        i = len(mats) // 2
        mats[i]["diffuse"]["color"] = np.array([0.125, 0.75, 0.25], np.float32)
        mats[i]["reflection"]["color"] = np.float32(0.0 if mats[i]["reflection"]["color"].any() else 0.375)
        out["materials"] = (i, mats[i:i + 1].copy())
    inst = hip.blob_table(blob, "instances")
    nodes = [k for k in range(1, len(inst)) if inst[k]["obj_type"] != 0]
    deep = [k for k in nodes if inst[k]["depth"] == 2]
    if nodes:
        k = deep[0] if deep else nodes[0]
        R = rotation(20.0, (1, 2, 3))
        tm = inst[k]["tm"].reshape(3, 3).T     # column-major storage
        itm = inst[k]["itm"].reshape(3, 3).T
        inst[k]["tm"] = (R @ tm).T.reshape(9)
        inst[k]["itm"] = (itm @ R.T).T.reshape(9)
        inst[k]["pos"] = R @ inst[k]["pos"] + np.array([0.25, -0.125, 0.0625], np.float32)
        out["instances"] = (k, inst[k:k + 1].copy())
    return out


def scene_b(name, size, tmp_path):
    """-> (blob B, camera record of B, the records of patch_records): B is the flattened XML copy with the moved camera, patched."""
    cam = moved_camera(xml_camera(scene_path(name)))
    dst = os.path.join(str(tmp_path), "moved_" + name)
    write_xml_with_camera(scene_path(name), dst, cam, size)
    from qaray_amd.host import HostScene, SCENES_DIR
    s = HostScene(dst, asset_root=SCENES_DIR)
    try:
        blob = s.flatten()
    finally:
        s.close()
    a = host_scene(name, size)
    try:
        a.set_camera(cam["pos"], cam["target"], cam["up"], cam["fov"], cam["focaldist"], cam["dof"])
        record = a.camera().copy()
    finally:
        a.close()
    return blob, record, patch_records(blob), cam


def apply_edits(ctx, record, records):
    ctx.edit_camera(record)
    if "lights" in records:
        ctx.edit_lights(*records["lights"])
    if "materials" in records:
        ctx.edit_materials(*records["materials"])
    if "instances" in records:
        ctx.edit_instances(*records["instances"])
