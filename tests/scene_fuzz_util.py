"""Deterministic generator of the scene-content fuzz cases (tests/test_scene_fuzz_host.py, tests/golden/make_goldens.py
scene_fuzz).

write_scene(dir, family, seed) writes <family>_<seed>.xml and its assets (cube.obj, hf.obj, tex.ppm) under dir and returns
the XML's path; params(family, seed) gives the frame (width, height, spp_min, spp_max, bounce).  The draws come from
np.random.default_rng with fixed seeds and every number is written with %.9g, so the text is the same everywhere
(tests/golden/scene_fuzz/manifest.json records its sha256).  The reference's own loader reads these files: only what its
xmlload.cpp parses is used.  Every seed of a family carries that family's edge values (the lists below); what cannot share a
scene (bounce limits, frame shapes, one camera, light counts) goes round the seeds.

Not generated, because the HIP path refuses them: nesting deeper than 8, partial texture vertices, area lights
with max_bounce above 7; nor a camera whose target is its position.
"""
import os

import numpy as np

FAMILIES = {"transforms": 4, "dielectric": 4, "lobes": 4, "lights": 11, "camera": 7, "contact": 4, "big": 4}
INDICES = (1, 0.5, 0.999, 1.0001, 1.33, 2.4, 10)          # refraction indices every dielectric seed carries
DEPTHS = (1, 2, 7, 8)                                      # transforms: nesting depth by seed (8 = QA_MAX_NODE_DEPTH)
BOUNCES = (0, 1, 5, 7)                                     # dielectric: max_bounce by seed
# lights: (shadow-casting lights, some of them with a size) by seed; 0 lights: none at all, then ambient only
LIGHT_SEEDS = ((0, 0), (0, 0), (1, 0), (1, 1), (4, 0), (4, 1), (5, 0), (6, 0), (6, 1), (9, 0), (9, 1))
# big: the family and seed whose scene gets the height-field mesh of 4608 triangles
BIG_OF = (("dielectric", 2), ("dielectric", 3), ("lights", 7), ("lights", 5))
FRAMES = ((48, 36), (37, 52), (52, 37), (45, 33))
SPPS = ((2, 2), (3, 3), (2, 5), (4, 4))                    # the third is adaptive


def cases():
    return [(f, s) for f, n in FAMILIES.items() for s in range(n)]


def params(family, seed):
    w, h = FRAMES[seed % 4]
    smin, smax = SPPS[(seed + (family == "lobes")) % 4]
    bounce = 5
    if family == "dielectric":
        bounce = BOUNCES[seed]
    if family == "big":
        f, s = BIG_OF[seed]
        bounce = params(f, s)["bounce"]
    if family == "lights" and LIGHT_SEEDS[seed][1]:
        bounce = (7, 3, 5, 7)[seed % 4]
        smin, smax = 2, (4 if seed == 5 else 2)
    if family == "camera":
        if seed == 5:
            w, h = 1, 36
        if seed == 6:
            w, h = 48, 1
    return dict(width=w, height=h, spp_min=smin, spp_max=smax, bounce=bounce)


def g(x):
    return "%.9g" % float(x)


def _attrs(names, vals):
    return "".join(' %s="%s"' % (n, g(v)) for n, v in zip(names, vals))


def scale(x, y=None, z=None):
    return '<scale value="%s"/>' % g(x) if y is None else "<scale%s/>" % _attrs("xyz", (x, y, z))


def rotate(angle, x, y, z):
    return '<rotate angle="%s"%s/>' % (g(angle), _attrs("xyz", (x, y, z)))


def translate(x, y, z):
    return "<translate%s/>" % _attrs("xyz", (x, y, z))


def obj(kind, name, material, *transforms, children=""):
    t = ' type="%s"' % kind if kind else ""
    m = ' material="%s"' % material if material else ""
    return '<object%s name="%s"%s>%s%s</object>' % (t, name, m, children, "".join(transforms))


def colour(tag, c, extra="", inner=""):
    if np.isscalar(c):
        a = ' value="%s"' % g(c)
    else:
        a = _attrs("rgb", c)
    return "<%s%s%s>%s</%s>" % (tag, a, extra, inner, tag) if inner else "<%s%s%s/>" % (tag, a, extra)


def blinn(name, diffuse=0.5, specular=0.3, gloss=20, emission=None, reflection=None, refl_gloss=None, refraction=None,
          index=None, refr_gloss=None, absorption=None, diffuse_extra="", diffuse_inner=""):
    s = '<material type="blinn" name="%s">' % name
    s += colour("diffuse", diffuse, diffuse_extra, diffuse_inner) + colour("specular", specular) + '<glossiness value="%s"/>' % g(gloss)
    if emission is not None:
        s += colour("emission", emission)
    if reflection is not None:
        s += colour("reflection", reflection, "" if refl_gloss is None else ' glossiness="%s"' % g(refl_gloss))
    if refraction is not None:
        e = "" if index is None else ' index="%s"' % g(index)
        e += "" if refr_gloss is None else ' glossiness="%s"' % g(refr_gloss)
        s += colour("refraction", refraction, e)
    if absorption is not None:
        s += colour("absorption", absorption)
    return s + "</material>"


def point(name, intensity, pos, size=None):
    return ('<light type="point" name="%s">%s<position%s/>%s</light>'
            % (name, colour("intensity", intensity), _attrs("xyz", pos), "" if size is None else '<size value="%s"/>' % g(size)))


def direct(name, intensity, d):
    return '<light type="direct" name="%s">%s<direction%s/></light>' % (name, colour("intensity", intensity), _attrs("xyz", d))


def ambient(name, intensity):
    return '<light type="ambient" name="%s">%s</light>' % (name, colour("intensity", intensity))


def spot(name, intensity, pos, rot, angle, blend, size=None, blend_first=False):
    a, b = '<angle value="%s"/>' % g(angle), '<blend value="%s"/>' % g(blend)
    return ('<light type="spot" name="%s">%s<position%s/><rotation angle="%s"%s/>%s%s</light>'
            % (name, colour("intensity", intensity), _attrs("xyz", pos), g(rot[0]), _attrs("xyz", rot[1:]),
               (b + a) if blend_first else (a + b), "" if size is None else '<size value="%s"/>' % g(size)))


def camera(pos, target, up=(0, 0, 1), fov=40, w=48, h=36, focaldist=None, dof=None):
    s = "<camera><position%s/><target%s/><up%s/>" % (_attrs("xyz", pos), _attrs("xyz", target), _attrs("xyz", up))
    s += '<fov value="%s"/>' % g(fov)
    if focaldist is not None:
        s += '<focaldist value="%s"/><dof value="%s"/>' % (g(focaldist), g(dof))
    return s + '<width value="%d"/><height value="%d"/></camera>' % (w, h)


def write_cube(d):
    """12 triangles, 8 vertices, one normal per face; two nodes of a scene share it."""
    v = [(x, y, z) for z in (-1, 1) for y in (-1, 1) for x in (-1, 1)]
    quads = [((0, 2, 3, 1), (0, 0, -1)), ((4, 5, 7, 6), (0, 0, 1)), ((0, 1, 5, 4), (0, -1, 0)), ((2, 6, 7, 3), (0, 1, 0)),
             ((0, 4, 6, 2), (-1, 0, 0)), ((1, 3, 7, 5), (1, 0, 0))]
    with open(os.path.join(d, "cube.obj"), "w") as f:
        for p in v:
            f.write("v %d %d %d\n" % p)
        for _, n in quads:
            f.write("vn %d %d %d\n" % n)
        for k, (q, _) in enumerate(quads):
            a, b, c, e = (i + 1 for i in q)
            f.write("f %d//%d %d//%d %d//%d\nf %d//%d %d//%d %d//%d\n" % (a, k + 1, b, k + 1, c, k + 1, a, k + 1, c, k + 1, e, k + 1))


def write_height_field(d, n=48):
    """The height field of tests/test_gpu_variant_census.py: 2 n^2 = 4608 triangles with texture vertices, not LDS-resident.
    Here with vertex normals (the surface's gradient): the reference computes missing normals in a loop over the faces on an
    array sized by the vertices (TriMesh::ComputeNormals), which overruns the heap for any mesh with more faces than vertices."""
    with open(os.path.join(d, "hf.obj"), "w") as f:
        for j in range(n + 1):
            for i in range(n + 1):
                x, y = -4 + 8 * i / n, -4 + 8 * j / n
                nx, ny = -0.6 * 1.3 * np.cos(1.3 * x) * np.cos(0.9 * y), 0.6 * 0.9 * np.sin(1.3 * x) * np.sin(0.9 * y)
                f.write("v %.7g %.7g %.7g\nvt %.7g %.7g\nvn %.7g %.7g 1\n"
                        % (x, y, 1.2 + 0.6 * np.sin(1.3 * x) * np.cos(0.9 * y), i / n, j / n, nx, ny))
        for j in range(n):
            for i in range(n):
                a, b, c, e = j * (n + 1) + i + 1, j * (n + 1) + i + 2, (j + 1) * (n + 1) + i + 2, (j + 1) * (n + 1) + i + 1
                f.write("f %d/%d/%d %d/%d/%d %d/%d/%d\nf %d/%d/%d %d/%d/%d %d/%d/%d\n" % (a, a, a, b, b, b, c, c, c, a, a, a, c, c, c, e, e, e))


def write_texture(d):
    with open(os.path.join(d, "tex.ppm"), "wb") as f:
        f.write(b"P6 8 8 255\n" + bytes((37 * k + 11 * (k // 24)) % 256 for k in range(8 * 8 * 3)))


FLOOR = blinn("floor", (0.6, 0.6, 0.55), 0.2, 15, emission=0.03)
MATTE = blinn("matte", (0.7, 0.4, 0.3), 0.4, 30, emission=0.05)


def _chain(rng, depth, name, leaves, place, mirror_two_only=False):
    """`leaves` ((kind, name, material, own transforms), ...) at nesting depth `depth`: depth - 1 groups around them.  The 16
    steps below, innermost first, are dealt out over the levels in order (the leaves take the first share after their own
    transforms), so every depth composes the same steps with other roundings: axis ratios of 1e3 and translations of 1e3
    that a later step (at depths above 1: an outer node) undoes, mirrors on one axis and on two, rotations by 0, 180, 360 and
    -90 degrees about un-normalised axes and axes with zero components, a shrink to 1e-3 and a growth by 1e3."""
    a, b, c = rng.uniform(0.6, 1.6, 3)
    ax = rng.uniform(-3, 3, 3)
    steps = [scale(a, b, c),
             translate(1000, -1000, 1000),
             rotate(0, 0, 0, 1),
             scale(1000, 1, 1),
             rotate(360, 3, 4, 0),
             scale(0.001, 1, 1),
             translate(-1000, 1000, -1000),
             scale(1, 1, 1) if mirror_two_only else scale(-1, 1, 1),
             rotate(180, 0, 0, 2),
             rotate(-90, *(rng.uniform(1, 5) * np.ones(3))),
             scale(1, -1, -1),
             rotate(rng.uniform(-180, 180), *ax),
             scale(0.001),
             rotate(rng.uniform(0, 90), 0, rng.uniform(1, 7), 0),
             scale(1000),
             translate(*place)]
    chunks = np.array_split(np.arange(len(steps)), depth)
    xml = "".join(obj(kind, n, m, *(list(own) + [steps[i] for i in chunks[0]])) for kind, n, m, own in leaves)
    for level in range(1, depth):
        xml = obj(None, "%s_l%d" % (name, depth - level), None, *[steps[i] for i in chunks[level]], children=xml)
    return xml


def _transforms(rng, seed, p):
    depth = DEPTHS[seed]
    la = [("obj", "cube.obj", "matte", (scale(0.8), translate(-1.2, 0, 0))),
          ("sphere", "ball", "shiny", (scale(1, 0.7, 0.5), translate(1.3, 0.2, 0.3)))]
    lb = [("obj", "cube.obj", "shiny", (rotate(rng.uniform(0, 360), *rng.uniform(-1, 1, 3)), scale(0.5, 0.9, 0.7))),
          ("plane", "card", "matte", (scale(1.4), rotate(60, 1, 0, 0), translate(0, 1.5, 0.5)))]
    objs = [obj("plane", "floor", "floor", scale(1000)),
            obj("sphere", "dome", "floor", scale(1000), translate(0, 1150, 0)),
            obj("sphere", "speck", "shiny", scale(0.001), translate(0, -8, 0.001)),
            obj("sphere", "needle", "shiny", scale(0.004, 0.004, 4), rotate(30, 0, 5, 0), translate(0, -2, 2.5)),
            _chain(rng, depth, "a", la, (-2.6, 0.5, 2.2)), _chain(rng, depth, "b", lb, (2.8, 1.0, 2.0), True)]
    mtls = [FLOOR, MATTE, blinn("shiny", (0.3, 0.5, 0.7), 0.6, 50, emission=0.04, reflection=0.4)]
    lights = [ambient("amb", 0.1), point("p0", 60, (3, -8, 11)), direct("d0", 0.5, (1, 2, -3))]
    cam = camera((0.5, -13, 5.5), (0, 0, 1.8), fov=42, w=p["width"], h=p["height"])
    return objs, mtls, lights, cam, '<background r="0.2" g="0.3" b="0.4"/><environment value="0.3"/>'


def _glass(name, k, seed, index):
    """Material k of a dielectric seed: the refraction value goes 1, 0.5, 0; reflection + refraction + diffuse sum to 0, 1, more;
    absorption 0 and 1e3; both glossinesses 0 and 0.5."""
    value = (1, 0.5, 1, 0, 1, 0.5, 1)[(k + seed) % 7]
    kind = (k + 2 * seed) % 5
    absorption = (None, (1000, 0.5, 0), 0, None)[(k + seed) % 4]
    rg, tg = ((None, None), (0.5, None), (None, 0.5), (0, 0.5))[(k + seed // 2) % 4]
    if kind == 0:      # sums to more than 1
        return blinn(name, 0.7, 0.8, 60, reflection=0.5, refl_gloss=rg, refraction=value, index=index, refr_gloss=tg, absorption=absorption)
    if kind == 1:      # sums to 0: emission only
        return blinn(name, 0, 0, 20, emission=(0.3, 0.2, 0.4), reflection=0, refraction=0, index=index)
    if kind == 2:      # sums to 1
        return blinn(name, 0.3, 0.5, 40, reflection=0.2, refl_gloss=rg, refraction=0.5, index=index, refr_gloss=tg, absorption=absorption)
    return blinn(name, 0, 0.8, 60, refraction=value, index=index, refr_gloss=tg if kind == 4 else None, absorption=absorption)


def _dielectric(rng, seed, p):
    objs = [obj("plane", "floor", "floor", scale(30))]
    mtls = [FLOOR, MATTE]
    for k in range(7):
        index = INDICES[(k + 3 * seed) % 7]
        mtls.append(_glass("g%d" % k, k, seed, index))
        # spheres of radius 0.9 tangent to the floor
        objs.append(obj("sphere", "s%d" % k, "g%d" % k, scale(0.9), translate(-4.8 + 1.6 * k, rng.uniform(-1.5, 1.5), 0.9)))
    mtls += [blinn("clear", 0, 0.8, 80, refraction=1, index=1.5), blinn("water", 0.05, 0.5, 40, reflection=0.3, refraction=0.5, index=1.33),
             blinn("thin", 0, 0.6, 30, refraction=0.9, index=0.5, absorption=(0.2, 0, 0.1))]
    x = rng.uniform(-1, 1)
    objs += [obj("sphere", "outer", "clear", scale(1.4), translate(x, -3.5, 1.4)),
             obj("sphere", "inner", "thin", scale(0.6), translate(x + 0.2, -3.5, 1.3)),           # nested
             obj("sphere", "over", "water", scale(1.0), translate(x + 1.7, -3.2, 1.0)),             # overlaps `outer`
             obj("sphere", "kiss", "clear", scale(0.5), translate(x, -3.5, 3.3)),                   # tangent to `outer` at its top
             obj("sphere", "solid", "matte", scale(0.7), translate(-3, 2.5, 0.7)),
             obj("plane", "pane", "water", scale(5, 2.5, 1), rotate(90, 1, 0, 0), translate(0, 3.5, 2.5))]   # a glass plane
    pos = (0.3, -12, 4.5)
    if seed % 2:
        # the camera inside a glass sphere
        objs.append(obj("sphere", "bowl", "clear", scale(1.5), translate(pos[0] + 0.2, pos[1] + 0.1, pos[2] - 0.3)))
    lights = [ambient("amb", 0.2), point("p0", 50, (4, -7, 10)), point("p1", 30, (-6, -3, 7)), direct("d0", 0.4, (0.3, 1, -1))]
    cam = camera(pos, (0, 0, 1.2), fov=44, w=p["width"], h=p["height"])
    return objs, mtls, lights, cam, '<background r="0.3" g="0.4" b="0.5"/><environment r="0.5" g="0.5" b="0.6"/>'


def _lobes(rng, seed, p):
    mtls = [blinn("floor", (0.6, 0.6, 0.55), 0.2, 15, emission=0.03, reflection=0.3, refl_gloss=(0.5, None, 0.1, 0)[seed]),
            blinn("gl0", 0.5, 0.6, 0, emission=0.02),                                     # glossiness 0: pow(x, 0), pow(0, 0)
            blinn("gl1", 0.5, 0.6, 1),
            blinn("gl1e4", 0.4, 0.9, 10000, reflection=0.2),
            blinn("hot", 0.3, 1.5 + rng.uniform(0, 2), 25),                               # specular above 1
            blinn("lamp", 0, 0, 20, emission=(0.9, 0.7, 0.2)),                            # diffuse 0, specular 0: emission only
            blinn("red", (0.8, 0, 0), (0, 0.5, 0), 20, reflection=(0, 0.7, 0.7)),         # zero channels: luma can vanish per lobe
            blinn("blue", (0, 0, 0.9), 0.3, 20, refraction=(0, 0, 0.9), index=1.5),
            blinn("green", (0, 1e-6, 0), (0, 0.8, 0), 30, reflection=(0, 2e-5, 0)),       # lumas about the 1e-5 threshold
            blinn("mirror", 0, 0, 20, reflection=1)]
    names = ["gl0", "gl1", "gl1e4", "hot", "lamp", "red", "blue", "green", "mirror"]
    objs = [obj("plane", "floor", "floor", scale(30))]
    for k, n in enumerate(names):
        r = rng.uniform(0.6, 0.9)
        i = (k + 2 * seed) % 9
        objs.append(obj("sphere", "s%d" % k, n, scale(r), translate(-3.6 + 1.8 * (i % 5), -1.5 + 3.0 * (i // 5) + rng.uniform(-0.3, 0.3), r)))
    objs.append(obj("obj", "cube.obj", names[seed % 9], scale(0.7), rotate(rng.uniform(0, 90), 0, 0, 1), translate(4.5, -3.5, 0.7)))
    lights = [ambient("amb", 0.15), point("p0", 60, (2, -9, 10)), direct("d0", 0.6, (-1, 1, -2))]
    cam = camera((0, -13, 6), (0, 0, 0.8), fov=40, w=p["width"], h=p["height"])
    return objs, mtls, lights, cam, '<background r="0.25" g="0.3" b="0.35"/><environment value="0.4"/>'


def _light_pool(rng, sized):
    """Nine shadow-casting lights; a scene takes the first n of a rotation of them."""
    s = (lambda v: v) if sized else (lambda v: None)
    return [direct("axis", 0.5, (0, 0, -1)),                                                   # along an axis
            point("onfloor", 8, (1.5, -2.5, 0)),                                               # exactly on the floor plane
            spot("s0", 50, (-3, -4, 7), (20, 3, 6, 0), 0, 0, size=s(0.6)),                     # angle 0 (clamped to 2 degrees), axis un-normalised
            direct("skew", 0.4, (3, -4, -12)),                                                 # un-normalised
            point("inside", 30, (-2.5, 0.5, 1.0)),                                             # inside sphere `a`
            spot("s90", 40, (2, -5, 6), (-25, 0, 0.5, 0), 90, 1, blend_first=True),            # blend set before angle
            point("behind", 40, (0.5, 0.5, -3), size=s(1.0)),                                  # behind the floor plane
            spot("s180", 30, (0, 1, 8), (rng.uniform(-10, 10), 2, 2, 0), 180, 0, size=s(0.5)), # angle 180 (clamped to 89 degrees a side)
            point("cut", 35, (2.2, 0.8, 1.6), size=s(1.0) if sized else None)]                 # its sphere cuts sphere `b`


def _lights(rng, seed, p):
    n, sized = LIGHT_SEEDS[seed]
    pool = _light_pool(rng, sized)
    r = (2 * seed) % 9
    lights = (pool[r:] + pool[:r])[:n]
    if seed == 1 or seed % 3 == 0 and seed:
        lights.insert(min(1, len(lights)), ambient("amb", (0.2, 0.25, 0.3)))
    objs = [obj("plane", "floor", "floor", scale(30)),
            obj("sphere", "a", "matte", scale(1.2), translate(-2.5, 0.5, 1.2)),
            obj("sphere", "b", "shiny", scale(1.0), translate(2.0, 1.0, 1.0)),
            obj("obj", "cube.obj", "matte", scale(0.8), rotate(rng.uniform(0, 90), 0, 0, 1), translate(0, -2, 0.8)),
            obj("sphere", "c", "glass", scale(0.8), translate(rng.uniform(-1, 1), 2.5, 0.8))]
    mtls = [blinn("floor", (0.6, 0.6, 0.55), 0.2, 15, emission=0.1), MATTE, blinn("shiny", (0.3, 0.5, 0.7), 0.6, 50, emission=0.04, reflection=0.4),
            blinn("glass", 0.05, 0.8, 60, refraction=0.9, index=1.5)]
    cam = camera((0.5, -12, 6), (0, 0, 1), fov=42, w=p["width"], h=p["height"])
    return objs, mtls, lights, cam, '<background r="0.2" g="0.25" b="0.3"/><environment value="0.35"/>'


def _camera(rng, seed, p):
    objs = [obj("plane", "floor", "floor", scale(30)),
            obj("sphere", "a", "matte", scale(1.2), translate(-1.5, 0.5, 1.2)),
            obj("sphere", "b", "shiny", scale(1.0), translate(1.6, 1.0, 1.0)),
            obj("obj", "cube.obj", "matte", scale(0.8), rotate(rng.uniform(0, 90), 0, 0, 1), translate(0, -2, 0.8)),
            obj("sphere", "dome", "floor", scale(60))]
    mtls = [FLOOR, MATTE, blinn("shiny", (0.3, 0.5, 0.7), 0.6, 50, emission=0.04, reflection=0.4)]
    lights = [ambient("amb", 0.1), point("p0", 60, (3, -8, 11)), direct("d0", 0.5, (1, 2, -3))]
    pos, tgt, kw = np.array((0.5, -12.0, 5.0)), np.array((0.0, 0.0, 1.0)), dict(fov=40)
    if seed == 0:
        kw = dict(fov=1)
        tgt = np.array((-1.5, 0.5, 1.9))
    elif seed == 1:
        kw = dict(fov=170)
    elif seed == 2:
        d = (tgt - pos) / np.linalg.norm(tgt - pos)
        side = np.cross(d, (0, 0, 1.0))
        kw = dict(fov=40, up=tuple(d + 5e-4 * side / np.linalg.norm(side)))        # up within 1e-3 rad of the view direction
    elif seed == 3:
        kw = dict(fov=40, focaldist=0.5, dof=2.0)                                  # large lens, focus right in front of it
    elif seed == 4:
        pos, tgt = np.array((0.0, -9.0, 0.0)), np.array((0.0, 0.0, 1.5))           # exactly on the floor plane
    elif seed == 5:
        kw = dict(fov=30)
    elif seed == 6:
        # one row of 48 pixels: fov is the height's, so 4 degrees already span 118 across; the row crosses both spheres
        kw = dict(fov=4)
        tgt = np.array((0.5, 0.8, 1.0))
    cam = camera(tuple(pos), tuple(tgt), w=p["width"], h=p["height"], **kw)
    return objs, mtls, lights, cam, '<background r="0.2" g="0.3" b="0.4"/><environment value="0.3"/>'


def _contact(rng, seed, p):
    checker = ' texture="checkerboard"', '<color1 r="0.1" g="0.1" b="0.2"/><color2 r="0.9" g="0.8" b="0.7"/><scale value="0.1"/>'
    mtls = [FLOOR, MATTE, blinn("check", 0.8, 0.2, 15, diffuse_extra=checker[0], diffuse_inner=checker[1]),
            blinn("globe", 0.9, 0.3, 30, emission=0.05, diffuse_extra=' texture="tex.ppm"'),
            blinn("shiny", (0.3, 0.5, 0.7), 0.6, 50, emission=0.04, reflection=0.4),
            blinn("glass", 0.05, 0.8, 60, refraction=0.9, index=1.5)]
    j = rng.uniform(-0.2, 0.2, 4)
    objs = [obj("plane", "floor", "floor", scale(30)),
            obj("plane", "floor2", "check", scale(30)),                                           # coincident, other material: a tie
            obj("sphere", "globe", "globe", scale(1.5), translate(0, 0, 1.5)),                    # tangent to both; its poles on the view axis
            obj("sphere", "t", "shiny", scale(1.0), translate(3 + j[0], j[1], 1.0)),              # tangent to the floor
            obj("sphere", "twin0", "matte", scale(0.9), translate(-3 + j[2], 1, 0.9)),
            obj("sphere", "twin1", "glass", scale(0.9), translate(-3 + j[2], 1, 0.9)),            # the same primitive twice at one place
            obj("obj", "cube.obj", "matte", scale(0.7), rotate(30 + 10 * seed, 0, 0, 1), translate(0.5, -3 + j[3], 0.7)),
            obj("obj", "cube.obj", "shiny", scale(0.7), rotate(30 + 10 * seed, 0, 0, 1), translate(0.5, -3 + j[3], 0.7))]
    lights = [ambient("amb", 0.1), point("p0", 50, (3, -6, 10)), direct("d0", 0.4, (1, 1, -3))]
    # straight down the globe's axis (its poles), from four heights / with and without a slight offset
    pos = ((0, 0, 14), (0, 0, 9), (1e-3, -1e-3, 12), (0, 0, 20))[seed]
    cam = camera(pos, (0, 0, 1.5), up=(0, 1, 0), fov=(40, 60, 45, 28)[seed], w=p["width"], h=p["height"])
    return objs, mtls, lights, cam, '<background r="0.2" g="0.3" b="0.4"/><environment value="0.3"/>'


_FAMILY = dict(transforms=_transforms, dielectric=_dielectric, lobes=_lobes, lights=_lights, camera=_camera, contact=_contact)
_FAMILY_ID = dict(transforms=1, dielectric=2, lobes=3, lights=4, camera=5, contact=6, big=7)


def write_scene(d, family, seed):
    p = params(family, seed)
    extra, base, bseed = [], family, seed
    if family == "big":
        base, bseed = BIG_OF[seed]
        write_height_field(d)
        extra = [obj("obj", "hf.obj", "hf", scale(0.6), rotate(15 * seed, 0, 0, 1), translate(0.5, 5.5, 0.4))]
    rng = np.random.default_rng(100 * _FAMILY_ID[base] + bseed)
    write_cube(d)
    write_texture(d)
    objs, mtls, lights, cam, sky = _FAMILY[base](rng, bseed, p)
    if extra:
        mtls = mtls + [blinn("hf", (0.3, 0.6, 0.8), 0.4, 25, emission=0.08, reflection=0.3)]
    xml = "<xml><scene>" + sky + "".join(objs + extra) + "".join(mtls) + "".join(lights) + "</scene>" + cam + "</xml>\n"
    path = os.path.join(d, "%s_%d.xml" % (family, seed))
    with open(path, "w") as f:
        f.write(xml)
    return path


def asset_names(family):
    return ["cube.obj", "tex.ppm"] + (["hf.obj"] if family == "big" else [])


# ---- what test modules share: the recorded reference results and one oracle frame per case ---------------------------
MANIFEST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scene_fuzz", "manifest.json")
_manifest, _frames, _tmp = None, {}, None


def manifest():
    """{(family, seed): entry} of tests/golden/scene_fuzz/manifest.json (written by tests/golden/make_goldens.py scene_fuzz)."""
    global _manifest
    if _manifest is None:
        import json
        with open(MANIFEST) as f:
            _manifest = {(e["family"], e["seed"]): e for e in json.load(f)["cases"]}
    return _manifest


def live_cases():
    return [c for c in cases() if "dropped" not in manifest().get(c, {})]


def case_id(c):
    return "%s_%d" % c


def sha(b):
    import hashlib
    return hashlib.sha256(b).hexdigest()


def scene_dir(family, seed):
    """The case's files, generated once per process."""
    global _tmp
    if _tmp is None:
        import tempfile
        _tmp = tempfile.TemporaryDirectory(prefix="scene_fuzz_")
    d = os.path.join(_tmp.name, "%s_%d" % (family, seed))
    if not os.path.isdir(d):
        os.makedirs(d)
        write_scene(d, family, seed)
    return d, os.path.join(d, "%s_%d.xml" % (family, seed))


def oracle_frame(family, seed):
    """-> dict(blob, rgb, depth, ns, cnt, params): the case's flat scene and the oracle's frame of it, computed once and shared."""
    if (family, seed) not in _frames:
        from oracle import binding as oracle
        from qaray_amd.host import load_scene_blob
        from qaray_amd.seed import DEFAULT_SEED
        d, xml = scene_dir(family, seed)
        p = params(family, seed)
        blob = load_scene_blob(xml, size=(p["width"], p["height"]), asset_root=d)
        rgb, depth, ns, cnt = oracle.render(blob, (0, 0, p["width"], p["height"]), p["spp_min"], max_bounce=p["bounce"],
                                            seed=DEFAULT_SEED, spp_max=p["spp_max"])
        for a in (blob, rgb, depth, ns):
            a.setflags(write=False)
        _frames[(family, seed)] = dict(blob=blob, rgb=rgb, depth=depth, ns=ns, cnt=cnt, params=p)
    return _frames[(family, seed)]
