"""ctypes binding of libqaray_hip.so (include/qaray_hip.h) - the MI355X integrator.

There is no CPU fallback: creating a context without the library or without a GPU raises."""
import collections
import ctypes as C
import os

import numpy as np

# (No environment variable is changed here.  The staged integrator's tile groups - Context.set_option("staged_groups", 4) -
# only pay when the PROCESS exported GPU_MAX_HW_QUEUES=8 before the HIP runtime initialised: bench.py and the tools do.)

_HERE = os.path.dirname(os.path.abspath(__file__))
HIP_LIB_PATH = os.environ.get("QA_HIP_LIB") or os.path.join(_HERE, "lib", "libqaray_hip.so")  # QA_HIP_LIB: A/B builds

QA_RENDER_STATS = 1
DEFAULT_SEED = 0x51A7A7


class Counters(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("casts_normal", C.c_uint64), ("casts_shadow", C.c_uint64),
                ("bvh_nodes", C.c_uint64), ("tri_tests", C.c_uint64), ("pixels", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class PhotonMapParams(C.Structure):   # include/qa_photon.h
    _fields_ = [("size", C.c_uint32), ("bounce", C.c_uint32), ("radius", C.c_float)]


class PhotonParams(C.Structure):
    _fields_ = [("photon", PhotonMapParams), ("caustics", PhotonMapParams)]


# qa_photon: byte-compatible with the reference's cy::PhotonMap::Photon (24 bytes)
PHOTON_DTYPE = np.dtype([("pos", np.float32, 3), ("power", np.float32), ("rgb", np.uint8, 3), ("plane_dirz", np.uint8),
                         ("dirx", np.int16), ("diry", np.int16)])


# the records of include/qa_flat_scene.h that Context.edit_* take (and blob_table views of a blob)
CAMERA_DTYPE = np.dtype([("screenA", np.float32, 3), ("screenU", np.float32, 3), ("screenV", np.float32, 3), ("screenX", np.float32, 3),
                         ("screenY", np.float32, 3), ("cam_pos", np.float32, 3), ("dof", np.float32)])
TEXCOLOR_DTYPE = np.dtype([("color", np.float32, 3), ("texmap", np.int32)])
LIGHT_DTYPE = np.dtype([("type", np.int32), ("intensity", np.float32, 3), ("position", np.float32, 3), ("direction", np.float32, 3),
                        ("size", np.float32), ("inner", np.float32), ("outer", np.float32), ("pad", np.int32, 3)])
MATERIAL_DTYPE = np.dtype([("diffuse", TEXCOLOR_DTYPE), ("specular", TEXCOLOR_DTYPE), ("reflection", TEXCOLOR_DTYPE),
                           ("refraction", TEXCOLOR_DTYPE), ("emission", TEXCOLOR_DTYPE), ("absorption", np.float32, 3),
                           ("ior", np.float32), ("kill", np.float32), ("gloss_spec", np.float32), ("gloss_refl", np.float32),
                           ("gloss_refr", np.float32)])
INSTANCE_DTYPE = np.dtype([("tm", np.float32, 9), ("itm", np.float32, 9), ("pos", np.float32, 3), ("obj_type", np.int32),
                           ("mesh", np.int32), ("mtlset", np.int32), ("parent", np.int32), ("subtree_end", np.int32),
                           ("depth", np.int32), ("pad", np.int32)])
TEXMAP_DTYPE = np.dtype([("itm", np.float32, 9), ("pos", np.float32, 3), ("texture", np.int32), ("pad", np.int32, 3)])
TEXTURE_DTYPE = np.dtype([("type", np.int32), ("width", np.int32), ("height", np.int32), ("pad0", np.int32), ("color1", np.float32, 3),
                          ("color2", np.float32, 3), ("off_texels", np.uint64), ("pad1", np.uint64)])
MTLSET_DTYPE = np.dtype([("first", np.int32), ("count", np.int32), ("multi", np.int32), ("pad", np.int32)])
MESH_DTYPE = np.dtype([("bmin", np.float32, 3), ("bmax", np.float32, 3), ("num_faces", np.uint32), ("num_vertices", np.uint32),
                       ("num_normals", np.uint32), ("num_texcoords", np.uint32), ("num_bvh_nodes", np.uint32), ("pad", np.uint32),
                       ("off_bvh_nodes", np.uint64), ("off_elements", np.uint64), ("off_faces", np.uint64), ("off_vertices", np.uint64),
                       ("off_normals", np.uint64), ("off_texcoords", np.uint64)])
FACE_DTYPE = np.dtype([("v", np.int32, 3), ("vn", np.int32, 3), ("vt", np.int32, 3), ("mtl", np.int32)])
assert (CAMERA_DTYPE.itemsize, LIGHT_DTYPE.itemsize, MATERIAL_DTYPE.itemsize, INSTANCE_DTYPE.itemsize) == (76, 64, 112, 112)
assert (TEXCOLOR_DTYPE.itemsize, TEXMAP_DTYPE.itemsize, TEXTURE_DTYPE.itemsize) == (16, 64, 56)
assert (MESH_DTYPE.itemsize, FACE_DTYPE.itemsize) == (96, 40)
QA_TEX_CHECKER, QA_TEX_FILE = 0, 1
# qa_flat_header: byte offsets of the counts and table offsets the views below need
_HEADER = {"camera": 16, "backdrop": 104, "instances": (136, 168), "meshes": (140, 176), "mtlsets": (144, 184), "materials": (148, 192), "lights": (152, 200), "texmaps": (156, 208),
           "textures": (160, 216)}
_TABLE_DTYPES = {"instances": INSTANCE_DTYPE, "meshes": MESH_DTYPE, "mtlsets": MTLSET_DTYPE, "materials": MATERIAL_DTYPE, "lights": LIGHT_DTYPE, "texmaps": TEXMAP_DTYPE,
                 "textures": TEXTURE_DTYPE}


def blob_camera(blob):
    """The camera block of a flat scene blob (numpy uint8) as a writable 0-d view of CAMERA_DTYPE (cam[...] = record)."""
    return blob[16:16 + CAMERA_DTYPE.itemsize].view(CAMERA_DTYPE).reshape(())


def blob_backdrop(blob):
    """The header's background and environment of a flat scene blob (numpy uint8) -> two writable 0-d views of TEXCOLOR_DTYPE."""
    at = _HEADER["backdrop"]
    both = blob[at:at + 2 * TEXCOLOR_DTYPE.itemsize].view(TEXCOLOR_DTYPE)
    return both[0:1].reshape(()), both[1:2].reshape(())


def blob_texels(blob, i):
    """The texels of file texture i of a flat scene blob (numpy uint8) as a writable (height, width, 3) uint8 view."""
    t = blob_table(blob, "textures")[i]
    assert t["type"] == QA_TEX_FILE, "a checker texture has no texels"
    w, h, off = int(t["width"]), int(t["height"]), int(t["off_texels"])
    return blob[off:off + 3 * w * h].reshape(h, w, 3)


def blob_mesh_arrays(blob, mesh):
    """The raw arrays of mesh `mesh` of a flat scene blob (numpy uint8) as writable views -> dict faces (FACE_DTYPE), vertices (nv, 3),
    normals (nn, 3), texcoords (nt, 2) float32."""
    m = blob_table(blob, "meshes")[mesh]

    def view(off, count, dtype, width):
        off, count = int(off), int(count)
        a = blob[off:off + count * width * np.dtype(dtype).itemsize].view(dtype)
        return a if width == 1 else a.reshape(count, width)
    return {"faces": view(m["off_faces"], m["num_faces"], FACE_DTYPE, 1), "vertices": view(m["off_vertices"], m["num_vertices"], np.float32, 3),
            "normals": view(m["off_normals"], m["num_normals"], np.float32, 3), "texcoords": view(m["off_texcoords"], m["num_texcoords"], np.float32, 2)}


def blob_table(blob, which):
    """The 'lights' / 'materials' / 'mtlsets' / 'instances' / 'meshes' / 'texmaps' / 'textures' table of a flat scene blob (numpy uint8) as a
    writable structured view."""
    at_count, at_off = _HEADER[which]
    n = int(blob[at_count:at_count + 4].view(np.uint32)[0])
    off = int(blob[at_off:at_off + 8].view(np.uint64)[0])
    dt = _TABLE_DTYPES[which]
    return blob[off:off + n * dt.itemsize].view(dt)


class DisplayStats(C.Structure):   # qa_display_stats
    _fields_ = [("zmin", C.c_float), ("zmax", C.c_float), ("smin", C.c_uint32), ("smax", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class DenoiseParams(C.Structure):   # qa_denoise_params; DenoiseParams.default() = qa_denoise_params_default
    _fields_ = [("iterations", C.c_int), ("sigma_color", C.c_float), ("sigma_depth", C.c_float), ("flags", C.c_uint32)]

    @classmethod
    def default(cls):
        p = cls()
        _check(lib().qa_denoise_params_default(C.byref(p)))
        return p

    @classmethod
    def of(cls, params=None, iterations=None, sigma_color=None, sigma_depth=None):
        """params (a DenoiseParams) or the library's defaults, with the keyword arguments that are given written over them."""
        return _params_of(cls, params, dict(iterations=iterations, sigma_color=sigma_color, sigma_depth=sigma_depth))


QA_DENOISE_GUIDE_NORMAL, QA_DENOISE_GUIDE_ALBEDO = 1, 2
QA_RADIANCE_PER_SAMPLE, QA_RADIANCE_MISS_ENVIRONMENT = 1, 2
QA_RADIANCE_PHOTON_MAPS = 8   # (bit 3: the batch gathers from the built photon maps, as a frame does)


class RadianceParams(C.Structure):   # qa_radiance_params; RadianceParams.default() = qa_radiance_params_default
    _fields_ = [("spp", C.c_int), ("max_bounce", C.c_int), ("seed", C.c_uint32), ("flags", C.c_uint32)]

    @classmethod
    def default(cls):
        p = cls()
        _check(lib().qa_radiance_params_default(C.byref(p)))
        return p

    @classmethod
    def of(cls, spp=None, max_bounce=None, seed=None, per_sample=False, miss_environment=False, photon_maps=False):
        """The library's defaults with the arguments that are given written over them."""
        p = cls.default()
        if spp is not None:
            p.spp = int(spp)
        if max_bounce is not None:
            p.max_bounce = int(max_bounce)
        if seed is not None:
            p.seed = int(seed) & 0xFFFFFFFF
        p.flags = ((QA_RADIANCE_PER_SAMPLE if per_sample else 0) | (QA_RADIANCE_MISS_ENVIRONMENT if miss_environment else 0) |
                   (QA_RADIANCE_PHOTON_MAPS if photon_maps else 0))
        return p


QA_PROBE_JITTER = 16   # (beside the radiance bits: QA_RADIANCE_PHOTON_MAPS is passed through)
QA_PROBE_MAX_M = 128


class ProbeParams(C.Structure):   # qa_probe_params; ProbeParams.default() = qa_probe_params_default
    _fields_ = [("m", C.c_int), ("spp", C.c_int), ("max_bounce", C.c_int), ("seed", C.c_uint32), ("flags", C.c_uint32), ("chunk_rays", C.c_uint64)]

    @classmethod
    def default(cls):
        p = cls()
        _check(lib().qa_probe_params_default(C.byref(p)))
        return p

    @classmethod
    def of(cls, m=None, spp=None, max_bounce=None, seed=None, jitter=False, photon_maps=False, chunk_rays=0):
        """The library's defaults with the arguments that are given written over them."""
        p = cls.default()
        if m is not None:
            p.m = int(m)
        if spp is not None:
            p.spp = int(spp)
        if max_bounce is not None:
            p.max_bounce = int(max_bounce)
        if seed is not None:
            p.seed = int(seed) & 0xFFFFFFFF
        p.flags = (QA_PROBE_JITTER if jitter else 0) | (QA_RADIANCE_PHOTON_MAPS if photon_maps else 0)
        p.chunk_rays = int(chunk_rays)
        return p


class ProbeVisParams(C.Structure):   # qa_probevis_params; ProbeVisParams.default() = qa_probevis_params_default
    _fields_ = [("d", C.c_int), ("dmax", C.c_float), ("normal_bias", C.c_float)]

    @classmethod
    def default(cls):
        p = cls()
        _check(lib().qa_probevis_params_default(C.byref(p)))
        return p

    @classmethod
    def of(cls, d=None, dmax=None, normal_bias=None):
        """The library's defaults (d 8, dmax 0 - which the calls refuse - normal_bias 0) with the arguments that are given written
        over them."""
        p = cls.default()
        if d is not None:
            p.d = int(d)
        if dmax is not None:
            p.dmax = float(dmax)
        if normal_bias is not None:
            p.normal_bias = float(normal_bias)
        return p


def _photon_maps_option(call, options):
    """The one keyword the point queries and bake_light take beyond their listed parameters: photon_maps (default False)."""
    unknown = sorted(set(options) - {"photon_maps"})
    if unknown:
        raise TypeError(f"{call}() got an unexpected keyword argument '{unknown[0]}'")
    return bool(options.get("photon_maps", False))


class DenoiseGuidedParams(C.Structure):   # qa_denoise_guided_params; .default() = qa_denoise_guided_params_default
    _fields_ = [("iterations", C.c_int), ("sigma_color", C.c_float), ("sigma_depth", C.c_float), ("sigma_normal", C.c_float), ("flags", C.c_uint32)]

    @classmethod
    def default(cls):
        p = cls()
        _check(lib().qa_denoise_guided_params_default(C.byref(p)))
        return p

    @classmethod
    def of(cls, params=None, flags=None, iterations=None, sigma_color=None, sigma_depth=None, sigma_normal=None):
        """params (a DenoiseGuidedParams) or the library's defaults, with the arguments that are given written over them."""
        return _params_of(cls, params, dict(flags=flags, iterations=iterations, sigma_color=sigma_color, sigma_depth=sigma_depth, sigma_normal=sigma_normal))


QA_DENOISE_GUIDE_VARIANCE = 4


class DenoiseVarianceParams(C.Structure):   # qa_denoise_variance_params; .default() = qa_denoise_variance_params_default
    _fields_ = [("iterations", C.c_int), ("sigma_color", C.c_float), ("sigma_depth", C.c_float), ("sigma_normal", C.c_float),
                ("variance_scale", C.c_float), ("flags", C.c_uint32)]

    @classmethod
    def default(cls):
        p = cls()
        _check(lib().qa_denoise_variance_params_default(C.byref(p)))
        return p

    @classmethod
    def of(cls, params=None, flags=None, iterations=None, sigma_color=None, sigma_depth=None, sigma_normal=None, variance_scale=None):
        """params (a DenoiseVarianceParams) or the library's defaults, with the arguments that are given written over them."""
        return _params_of(cls, params, dict(flags=flags, iterations=iterations, sigma_color=sigma_color, sigma_depth=sigma_depth, sigma_normal=sigma_normal,
                                            variance_scale=variance_scale))


def _params_of(cls, params, values, bits=()):
    """The override rule of the Denoise*Params.of and Reproject*Params.of: a copy of params (or cls.default()) with the values that
    are not None written over its fields (iterations, clamp_radius and flags as int, every other as float), and every (flag bit,
    bool or None) of bits set, cleared or left."""
    p = cls.default() if params is None else cls(*(getattr(params, name) for name, _ in cls._fields_))
    for name, v in values.items():
        if v is not None:
            setattr(p, name, int(v) if name in ("iterations", "clamp_radius", "flags") else float(v))
    for bit, v in bits:
        if v is not None:
            p.flags = (p.flags | bit) if v else (p.flags & ~bit)
    return p


class ReprojectParams(C.Structure):   # qa_reproject_params; ReprojectParams.default() = qa_reproject_params_default
    _fields_ = [("depth_tolerance", C.c_float), ("max_history", C.c_float), ("flags", C.c_uint32)]

    @classmethod
    def default(cls):
        p = cls()
        _check(lib().qa_reproject_params_default(C.byref(p)))
        return p

    @classmethod
    def of(cls, params=None, depth_tolerance=None, max_history=None):
        """params (a ReprojectParams) or the library's defaults, with the keyword arguments that are given written over them."""
        return _params_of(cls, params, dict(depth_tolerance=depth_tolerance, max_history=max_history))


QA_REPROJECT_MOTION, QA_REPROJECT_CLAMP = 1, 2
# qa_node_motion: m = a row-major 3x3 matrix and a translation, current world point -> where it lay in the previous scene
NODE_MOTION_DTYPE = np.dtype([("m", np.float32, 12), ("moved", np.uint32), ("pad", np.uint32, 3)])
assert NODE_MOTION_DTYPE.itemsize == 64


class ReprojectMotionParams(C.Structure):   # qa_reproject_motion_params; .default() = qa_reproject_motion_params_default
    _fields_ = [("depth_tolerance", C.c_float), ("max_history", C.c_float), ("clamp_gamma", C.c_float), ("clamp_radius", C.c_int32), ("flags", C.c_uint32)]

    @classmethod
    def default(cls):
        p = cls()
        _check(lib().qa_reproject_motion_params_default(C.byref(p)))
        return p

    @classmethod
    def of(cls, params=None, depth_tolerance=None, max_history=None, motion=None, clamp=None, clamp_radius=None, clamp_gamma=None):
        """params (a ReprojectMotionParams) or the library's defaults, with the keyword arguments that are given written over them;
        motion / clamp (bool) set or clear QA_REPROJECT_MOTION / QA_REPROJECT_CLAMP of the flags."""
        return _params_of(cls, params, dict(depth_tolerance=depth_tolerance, max_history=max_history, clamp_gamma=clamp_gamma, clamp_radius=clamp_radius),
                          ((QA_REPROJECT_MOTION, motion), (QA_REPROJECT_CLAMP, clamp)))


QA_REPROJECT_MOMENTS, QA_REPROJECT_SHORTEN = 4, 8


class ReprojectMomentsParams(C.Structure):   # qa_reproject_moments_params; .default() = qa_reproject_moments_params_default
    _fields_ = [("depth_tolerance", C.c_float), ("max_history", C.c_float), ("clamp_gamma", C.c_float), ("min_frames", C.c_float),
                ("shorten_rate", C.c_float), ("clamp_radius", C.c_int32), ("flags", C.c_uint32)]

    @classmethod
    def default(cls):
        p = cls()
        _check(lib().qa_reproject_moments_params_default(C.byref(p)))
        return p

    @classmethod
    def of(cls, params=None, depth_tolerance=None, max_history=None, motion=None, clamp=None, clamp_radius=None, clamp_gamma=None, moments=None,
           shorten=None, min_frames=None, shorten_rate=None):
        """params (a ReprojectMomentsParams) or the library's defaults, with the keyword arguments that are given written over them;
        motion / clamp / moments / shorten (bool) set or clear the four flags."""
        return _params_of(cls, params, dict(depth_tolerance=depth_tolerance, max_history=max_history, clamp_gamma=clamp_gamma, min_frames=min_frames,
                                            shorten_rate=shorten_rate, clamp_radius=clamp_radius),
                          ((QA_REPROJECT_MOTION, motion), (QA_REPROJECT_CLAMP, clamp), (QA_REPROJECT_MOMENTS, moments), (QA_REPROJECT_SHORTEN, shorten)))


QA_GBUFFER_BACKFACE = 0x40000000
GBUFFER_PLANES = ("normal", "albedo", "depth", "ids")   # in the C ABI's order: float32 [h,w,3], [h,w,3], [h,w], int32 [h,w,2]
MATTE_PLANES = ("coverage", "albedo", "normal", "backdrop")   # in the C ABI's order: float32 [h,w], [h,w,3], [h,w,3], [h,w,3]
# the id matte (qa_idmatte_dev.h): ids int32 [h,w,8], counts uint32 [h,w,8], other and samples uint32 [h,w], in the C ABI's order
IDMATTE_PLANES = ("ids", "counts", "other", "samples")
QA_IDMATTE_SLOTS = 8
QA_IDMATTE_EMPTY = -2 ** 31   # the id of a free slot: no key has it
QA_IDMATTE_NODE, QA_IDMATTE_MATERIAL = 0, 1
QA_IDMATTE_MAX_SELECT = 256
_IDMATTE_KEYS = {"node": QA_IDMATTE_NODE, "material": QA_IDMATTE_MATERIAL}
# ambient occlusion (qa_ao_dev.h): open and rays uint32 [h,w], ao float32 [h,w], in the C ABI's order
AO_PLANES = ("open", "rays", "ao")
QA_AO_MAX_RAYS = 256
BAKE_PLANES = ("point", "normal", "face", "bary")   # in the C ABI's order: float32 [h,w,3], [h,w,3], int32 [h,w], float32 [h,w,2]
QA_BAKE_MAX_DIM, QA_BAKE_MAX_RADIUS, QA_BAKE_MAX_TILES = 8192, 8, 4
QA_RAY_MISS = 1e30   # the t of a ray that hits nothing (exactly np.float32(1e30))
RAY_OUTPUTS = ("t", "ids", "normal", "point")   # in the C ABI's order: float32 [n], int32 [n,2], float32 [n,3], [n,3]
QA_MAX_RAYS = 2 ** 31 - 1


# Progressive.display(): numpy arrays shaped like the region (color [h,w,3], the others [h,w], uint8) and the statistics as a dict
Display = collections.namedtuple("Display", "color count zimg countimg mask stats")
DISPLAY_STATS_DTYPE = np.dtype([("zmin", np.float32), ("zmax", np.float32), ("smin", np.uint32), ("smax", np.uint32)])


class HipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libqaray_hip error {code}: {msg}")
        self.code = code


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(HIP_LIB_PATH):
            raise RuntimeError(
                f"{HIP_LIB_PATH} is missing: the HIP extension is the product path and has no fallback - "
                "build it with `python -c 'import __graft_entry__ as g; g.build()'` or `make -C qaray_amd/csrc hip`")
        # PyTorch wheels bundle their own HIP runtime (torch/lib/libamdhip64.so).  Two HIP runtimes in one
        # process do not share the device: whichever initialises second reports "No HIP GPUs are
        # available".  Loading torch first makes libqaray_hip.so bind to the runtime torch already
        # loaded, so device pointers and streams can be exchanged; without torch the system runtime is used.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(HIP_LIB_PATH)
        L.qa_last_error.restype = C.c_char_p
        L.qa_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        L.qa_ctx_destroy.argtypes = [C.c_void_p]
        L.qa_scene_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.qa_scene_upload_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.qa_render_region.argtypes = [C.c_void_p] + [C.c_int] * 7 + [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.qa_render_region_device.argtypes = [C.c_void_p] + [C.c_int] * 7 + [C.c_uint32, C.c_uint32, C.c_void_p,
                                                                            C.c_void_p, C.c_void_p, C.c_void_p]
        L.qa_render_strips_device.argtypes = [C.c_void_p] + [C.c_int] * 9 + [C.c_uint32, C.c_uint32, C.c_void_p,
                                                                            C.c_void_p, C.c_void_p, C.c_void_p]
        L.qa_strip_count.argtypes = [C.c_int] * 4
        L.qa_empty_tiles_device.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p, C.c_void_p]
        L.qa_test_empty_tiles_host.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p]
        L.qa_synchronize.argtypes = [C.c_void_p]
        L.qa_request_stop.argtypes = [C.c_void_p]
        L.qa_clear_stop.argtypes = [C.c_void_p]
        L.qa_get_counters.argtypes = [C.c_void_p, C.POINTER(Counters)]
        L.qa_reset_counters.argtypes = [C.c_void_p]
        L.qa_get_kernel_time.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
        L.qa_reset_kernel_time.argtypes = [C.c_void_p]
        L.qa_set_launch_config.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.qa_debug_scrub_scratch.argtypes = [C.c_void_p, C.c_uint32]
        L.qa_set_pipeline.argtypes = [C.c_void_p, C.c_int]
        L.qa_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_longlong]
        L.qa_get_kernel_name.argtypes = [C.c_void_p]
        L.qa_get_kernel_name.restype = C.c_char_p
        L.qa_get_staged_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        L.qa_progressive_begin.argtypes = [C.c_void_p] + [C.c_int] * 7 + [C.c_uint32, C.c_uint32]
        L.qa_progressive_advance.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.qa_progressive_read.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.qa_progressive_read_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.qa_progressive_status.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.qa_progressive_end.argtypes = [C.c_void_p]
        L.qa_display_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int] + [C.c_void_p] * 7
        L.qa_progressive_display.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.POINTER(DisplayStats)]
        L.qa_progressive_display_device.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 7
        L.qa_test_display_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int] + [C.c_void_p] * 6
        L.qa_denoise_params_default.argtypes = [C.POINTER(DenoiseParams)]
        L.qa_denoise_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(DenoiseParams), C.c_void_p,
                                        C.c_void_p]
        L.qa_progressive_denoise.argtypes = [C.c_void_p, C.POINTER(DenoiseParams), C.c_void_p]
        L.qa_progressive_denoise_device.argtypes = [C.c_void_p, C.POINTER(DenoiseParams), C.c_void_p, C.c_void_p]
        L.qa_test_denoise_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(DenoiseParams), C.c_void_p]
        L.qa_denoise_guided_params_default.argtypes = [C.POINTER(DenoiseGuidedParams)]
        L.qa_denoise_guided_device.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_int, C.POINTER(DenoiseGuidedParams), C.c_void_p, C.c_void_p]
        L.qa_progressive_denoise_guided.argtypes = [C.c_void_p, C.POINTER(DenoiseGuidedParams), C.c_void_p]
        L.qa_progressive_denoise_guided_device.argtypes = [C.c_void_p, C.POINTER(DenoiseGuidedParams), C.c_void_p, C.c_void_p]
        L.qa_test_denoise_guided_host.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_int, C.POINTER(DenoiseGuidedParams), C.c_void_p]
        L.qa_denoise_variance_params_default.argtypes = [C.POINTER(DenoiseVarianceParams)]
        L.qa_denoise_variance_device.argtypes = [C.c_void_p] * 7 + [C.c_int, C.c_int, C.POINTER(DenoiseVarianceParams), C.c_void_p, C.c_void_p]
        L.qa_test_denoise_variance_host.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_int, C.POINTER(DenoiseVarianceParams), C.c_void_p]
        L.qa_reproject_params_default.argtypes = [C.POINTER(ReprojectParams)]
        L.qa_reproject_device.argtypes = [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_void_p] * 8 + [C.POINTER(ReprojectParams)] + [C.c_void_p] * 3
        L.qa_progressive_reproject_device.argtypes = [C.c_void_p] * 6 + [C.POINTER(ReprojectParams)] + [C.c_void_p] * 3
        L.qa_test_reproject_host.argtypes = [C.c_void_p] * 2 + [C.c_int] * 4 + [C.c_void_p] * 8 + [C.POINTER(ReprojectParams)] + [C.c_void_p] * 2
        L.qa_reproject_motion_params_default.argtypes = [C.POINTER(ReprojectMotionParams)]
        L.qa_reproject_node_motion.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.qa_reproject_motion_device.argtypes = ([C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_void_p] * 9 + [C.c_int, C.POINTER(ReprojectMotionParams)]
                                                 + [C.c_void_p] * 3)
        L.qa_progressive_reproject_motion_device.argtypes = [C.c_void_p] * 7 + [C.c_int, C.POINTER(ReprojectMotionParams)] + [C.c_void_p] * 3
        L.qa_test_reproject_motion_host.argtypes = ([C.c_void_p] * 2 + [C.c_int] * 4 + [C.c_void_p] * 9 + [C.c_int, C.POINTER(ReprojectMotionParams)]
                                                    + [C.c_void_p] * 2)
        L.qa_reproject_moments_params_default.argtypes = [C.POINTER(ReprojectMomentsParams)]
        L.qa_reproject_moments_device.argtypes = ([C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_void_p] * 10 + [C.c_int, C.POINTER(ReprojectMomentsParams)]
                                                  + [C.c_void_p] * 5)
        L.qa_progressive_reproject_moments_device.argtypes = [C.c_void_p] * 8 + [C.c_int, C.POINTER(ReprojectMomentsParams)] + [C.c_void_p] * 5
        L.qa_test_reproject_moments_host.argtypes = ([C.c_void_p] * 2 + [C.c_int] * 4 + [C.c_void_p] * 10 + [C.c_int, C.POINTER(ReprojectMomentsParams)]
                                                     + [C.c_void_p] * 4)
        L.qa_gbuffer_region_device.argtypes = [C.c_void_p] + [C.c_int] * 4 + [C.c_uint32] + [C.c_void_p] * 5
        L.qa_gbuffer_region.argtypes = [C.c_void_p] + [C.c_int] * 4 + [C.c_uint32] + [C.c_void_p] * 4
        L.qa_progressive_gbuffer_device.argtypes = [C.c_void_p] * 6
        L.qa_matte_region_device.argtypes = [C.c_void_p] + [C.c_int] * 4 + [C.c_uint32] + [C.c_void_p] * 6
        L.qa_matte_region.argtypes = [C.c_void_p] + [C.c_int] * 4 + [C.c_uint32] + [C.c_void_p] * 5
        L.qa_progressive_matte_device.argtypes = [C.c_void_p] * 6
        L.qa_matte_rgba_device.argtypes = [C.c_void_p] * 5 + [C.c_uint64, C.c_int, C.c_void_p, C.c_void_p]
        L.qa_test_matte_accumulate_host.argtypes = [C.c_void_p] * 3 + [C.c_uint32] + [C.c_void_p] * 4
        L.qa_test_matte_rgba_host.argtypes = [C.c_void_p] * 4 + [C.c_uint64, C.c_int, C.c_void_p]
        L.qa_idmatte_region_device.argtypes = [C.c_void_p] + [C.c_int] * 4 + [C.c_uint32, C.c_void_p, C.c_int] + [C.c_void_p] * 5
        L.qa_idmatte_region.argtypes = [C.c_void_p] + [C.c_int] * 4 + [C.c_uint32, C.c_void_p, C.c_int] + [C.c_void_p] * 4
        L.qa_progressive_idmatte_device.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5
        L.qa_idmatte_select_device.argtypes = [C.c_void_p] * 4 + [C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.qa_test_idmatte_accumulate_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_void_p] * 3
        L.qa_test_idmatte_select_host.argtypes = [C.c_void_p] * 3 + [C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p]
        L.qa_ao_region_device.argtypes = [C.c_void_p] + [C.c_int] * 4 + [C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_float, C.c_uint32] + [C.c_void_p] * 4
        L.qa_ao_region.argtypes = [C.c_void_p] + [C.c_int] * 4 + [C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_float, C.c_uint32] + [C.c_void_p] * 3
        L.qa_progressive_ao_device.argtypes = [C.c_void_p, C.c_uint32, C.c_float] + [C.c_void_p] * 4
        L.qa_ao_points_device.argtypes = [C.c_void_p, C.c_uint64] + [C.c_void_p] * 3 + [C.c_uint32, C.c_uint32, C.c_float, C.c_uint32] + [C.c_void_p] * 3
        L.qa_ao_points.argtypes = [C.c_void_p, C.c_uint64] + [C.c_void_p] * 3 + [C.c_uint32, C.c_uint32, C.c_float, C.c_uint32] + [C.c_void_p] * 2
        L.qa_ao_grey_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.qa_test_ao_directions_host.argtypes = [C.c_uint32] + [C.c_void_p] * 3 + [C.c_uint64, C.c_void_p]
        L.qa_test_ao_face_normal_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        L.qa_test_ao_sphere_host.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.qa_test_ao_direction_from_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        L.qa_bake_texels_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint32] + [C.c_void_p] * 5
        L.qa_bake_texels.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint32] + [C.c_void_p] * 4
        L.qa_bake_dilate_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        L.qa_test_bake_texels_host.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint32] + [C.c_void_p] * 4
        L.qa_test_bake_dilate_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
        L.qa_cast_rays_device.argtypes = [C.c_void_p, C.c_uint64] + [C.c_void_p] * 7
        L.qa_cast_rays.argtypes = [C.c_void_p, C.c_uint64] + [C.c_void_p] * 6
        L.qa_occluded_device.argtypes = [C.c_void_p, C.c_uint64] + [C.c_void_p] * 5
        L.qa_occluded.argtypes = [C.c_void_p, C.c_uint64] + [C.c_void_p] * 4
        L.qa_camera_rays_device.argtypes = [C.c_void_p] + [C.c_int] * 4 + [C.c_uint32] + [C.c_void_p] * 3
        L.qa_radiance_params_default.argtypes = [C.POINTER(RadianceParams)]
        L.qa_radiance_rays_device.argtypes = [C.c_void_p, C.c_uint64] + [C.c_void_p] * 6 + [C.POINTER(RadianceParams)] + [C.c_void_p] * 4
        L.qa_radiance_rays.argtypes = [C.c_void_p, C.c_uint64] + [C.c_void_p] * 6 + [C.POINTER(RadianceParams)] + [C.c_void_p] * 3
        L.qa_camera_sample_rays_device.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 7
        L.qa_irradiance_points_device.argtypes = [C.c_void_p, C.c_uint64] + [C.c_void_p] * 3 + [C.POINTER(RadianceParams)] + [C.c_void_p] * 3
        L.qa_irradiance_points.argtypes = [C.c_void_p, C.c_uint64] + [C.c_void_p] * 3 + [C.POINTER(RadianceParams)] + [C.c_void_p] * 2
        L.qa_probe_params_default.argtypes = [C.POINTER(ProbeParams)]
        L.qa_probe_sh_device.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(ProbeParams)] + [C.c_void_p] * 5
        L.qa_probe_sh.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(ProbeParams)] + [C.c_void_p] * 4
        L.qa_probe_shade_device.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64] + [C.c_void_p] * 4
        L.qa_probe_grid_shade_device.argtypes = [C.c_void_p, C.c_uint64] + [C.c_void_p] * 8
        L.qa_test_probe_directions_host.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64] + [C.c_void_p] * 3
        L.qa_test_probe_project_host.argtypes = [C.c_uint64] + [C.c_void_p] * 7
        L.qa_test_probe_shade_host.argtypes = [C.c_uint64, C.c_void_p, C.c_uint64] + [C.c_void_p] * 3
        L.qa_test_probe_grid_shade_host.argtypes = [C.c_uint64] + [C.c_void_p] * 7
        L.qa_probevis_params_default.argtypes = [C.POINTER(ProbeVisParams)]
        L.qa_probevis_sh_device.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(ProbeParams), C.POINTER(ProbeVisParams)] + [C.c_void_p] * 6
        L.qa_probevis_sh.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(ProbeParams), C.POINTER(ProbeVisParams)] + [C.c_void_p] * 5
        L.qa_probevis_grid_shade_device.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.POINTER(ProbeVisParams)] + [C.c_void_p] * 2
        L.qa_test_probevis_moments_host.argtypes = [C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]
        L.qa_test_probevis_grid_shade_host.argtypes = [C.c_uint64, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.POINTER(ProbeVisParams), C.c_void_p]
        L.qa_reflprobe_layout.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 4
        L.qa_reflprobe_prefilter_device.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.qa_reflprobe_shade_device.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.c_int] + [C.c_void_p] * 5
        L.qa_reflprobe_grid_shade_device.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 8
        L.qa_test_reflprobe_prefilter_host.argtypes = [C.c_uint64, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.qa_test_reflprobe_shade_host.argtypes = [C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.c_int] + [C.c_void_p] * 4
        L.qa_test_reflprobe_grid_shade_host.argtypes = [C.c_uint64, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 7
        L.qa_scene_edit_camera.argtypes = [C.c_void_p, C.c_void_p]
        for name in ("qa_scene_edit_lights", "qa_scene_edit_materials", "qa_scene_edit_instances"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        for name in ("qa_scene_edit_texmaps", "qa_scene_edit_textures"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        L.qa_scene_edit_backdrop.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.qa_scene_edit_texels.argtypes = [C.c_void_p, C.c_uint32] + [C.c_int] * 4 + [C.c_void_p, C.c_uint64]
        L.qa_scene_edit_texels_device.argtypes = [C.c_void_p, C.c_uint32] + [C.c_int] * 4 + [C.c_void_p, C.c_uint64, C.c_void_p]
        L.qa_test_texels_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint64, C.c_void_p]
        L.qa_scene_download.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        L.qa_get_scene_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        L.qa_progressive_restart.argtypes = [C.c_void_p]
        L.qa_progressive_tile_count.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.qa_progressive_advance_tiles.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.qa_progressive_advance_tiles_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.qa_progressive_tile_levels.argtypes = [C.c_void_p, C.c_void_p]
        L.qa_progressive_tile_levels_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.qa_progressive_tile_error.argtypes = [C.c_void_p, C.c_void_p]
        L.qa_progressive_tile_error_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.qa_progressive_advance_adaptive.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_float, C.c_void_p]
        L.qa_progressive_adaptive_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        L.qa_progressive_state.argtypes = [C.c_void_p, C.c_void_p]
        L.qa_test_tile_error_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.qa_test_tile_select_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p, C.POINTER(C.c_uint64)]
        L.qa_photon_maps_build.argtypes = [C.c_void_p, C.POINTER(PhotonParams), C.c_uint32]
        L.qa_photon_maps_clear.argtypes = [C.c_void_p]
        L.qa_photon_maps_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.qa_photon_maps_download.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64]
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise HipError(rc, lib().qa_last_error().decode())


def tile_error_host(state):
    """qa_test_tile_error_host: the per-tile error map (Progressive.tile_error) of a state slab, uint32 [h,w,8] as
    Progressive.state() returns it, on the CPU from the source the device kernel is compiled from -> float32 [ty,tx].  No GPU needed."""
    if not isinstance(state, np.ndarray) or state.dtype != np.uint32 or state.ndim != 3 or state.shape[2] != 8 or state.shape[0] < 1 or state.shape[1] < 1:
        raise ValueError("state: a uint32 array of shape (h, w, 8) is expected")
    state = np.ascontiguousarray(state)
    h, w = state.shape[:2]
    out = np.zeros(((h + 7) // 8, (w + 7) // 8), np.float32)
    _check(lib().qa_test_tile_error_host(state.ctypes.data, w, h, out.ctypes.data))
    return out


def empty_tiles_host(blob, region, first_strip=0, strip_step=1):
    """qa_test_empty_tiles_host: the 8x8 tiles of `region` (its strips first_strip, first_strip + strip_step, ...) that a one-shot
    frame of a context with default options finishes in closed form, because no camera ray of theirs can hit anything (option
    'empty_tiles'), on the CPU from the source the kernel is compiled from -> bool [strips, tiles per strip].  All False for a scene
    that does not run on qa_integrate_lastcast with tile lists.  No GPU needed."""
    blob = np.ascontiguousarray(blob)
    x0, y0, x1, y1 = (int(v) for v in region)
    mask = np.zeros((strip_count(y0, y1, first_strip, strip_step), (x1 - x0 + 7) // 8), np.uint8)
    rc = lib().qa_test_empty_tiles_host(blob.ctypes.data, x0, y0, x1, y1, int(first_strip), int(strip_step), mask.ctypes.data)
    if rc != 0:
        raise HipError(rc, "qa_test_empty_tiles_host: bad scene or region")
    return mask.astype(bool)


def tile_select_host(error, levels, target, max_tiles=0, min_error=0.0):
    """qa_test_tile_select_host: the tiles Progressive.advance_adaptive(target, max_tiles, min_error=min_error) takes, given the
    tiles' error (float32) and levels (uint32) of one shape, on the CPU from the source the device kernel is compiled from ->
    (mask, bool of that shape; info dict as Progressive.adaptive_info, the two errors as their uint32 bits).  No GPU needed."""
    error = np.ascontiguousarray(error, dtype=np.float32)
    levels = np.ascontiguousarray(levels, dtype=np.uint32)
    if error.shape != levels.shape or error.size < 1:
        raise ValueError("error and levels must have one shape and at least one tile")
    if not min_error >= 0.0:
        raise ValueError("min_error must not be negative or a NaN")
    mask = np.zeros(error.shape, np.uint8)
    v = (C.c_uint64 * 4)()
    _check(lib().qa_test_tile_select_host(error.ctypes.data, levels.ctypes.data, error.size, int(target), int(max_tiles), float(min_error),
                                          mask.ctypes.data, v))
    return mask.astype(bool), {"selected": int(v[0]), "candidates": int(v[1]), "cut_bits": int(v[2]), "max_finite_bits": int(v[3])}


def display_host(rgb, depth, ns, spp_max, srgb=True):
    """qa_test_display_host: the 8-bit products of a frame of float results (any shape; rgb has 3 floats per pixel) on the CPU,
    from the source the device kernels are compiled from -> Display of flat uint8 arrays and the statistics.  No GPU needed."""
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    depth = np.ascontiguousarray(depth, dtype=np.float32)
    ns = np.ascontiguousarray(ns, dtype=np.uint32)
    n = depth.size
    assert rgb.size == 3 * n and ns.size == n
    out = [np.zeros(3 * n if k == 0 else n, np.uint8) for k in range(5)]
    st = DisplayStats()
    _check(lib().qa_test_display_host(rgb.ctypes.data, depth.ctypes.data, ns.ctypes.data, n, int(spp_max), int(bool(srgb)),
                                      *(a.ctypes.data for a in out), C.addressof(st)))
    return Display(*out, st.as_dict())


def matte_accumulate_host(values, normals, hit):
    """qa_test_matte_accumulate_host: one pixel's matte planes from its n samples on the CPU, from the source the device kernel is
    compiled from.  values (n, 3) f32: what gbuffer's albedo plane would hold for each sample's ray; normals (n, 3) f32: the hits'
    normals (read where hit is set); hit (n,) bool -> dict coverage () f32, albedo / normal / backdrop (3,) f32.  No GPU needed."""
    values = np.ascontiguousarray(values, dtype=np.float32).reshape(-1, 3)
    normals = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
    hit = np.ascontiguousarray(hit).astype(np.uint8).reshape(-1)
    n = len(hit)
    if values.shape != (n, 3) or normals.shape != (n, 3):
        raise ValueError(f"values and normals: shape ({n}, 3) is expected, not {values.shape} and {normals.shape}")
    out = {"coverage": np.zeros(1, np.float32), "albedo": np.zeros(3, np.float32), "normal": np.zeros(3, np.float32), "backdrop": np.zeros(3, np.float32)}
    _check(lib().qa_test_matte_accumulate_host(values.ctypes.data, normals.ctypes.data, hit.ctypes.data, n, *(out[k].ctypes.data for k in MATTE_PLANES)))
    out["coverage"] = out["coverage"].reshape(())
    return out


def matte_rgba_host(rgb, backdrop, coverage, ns, srgb=True):
    """qa_test_matte_rgba_host: the straight-alpha RGBA bytes of a frame (rgb, backdrop (.., 3) f32; coverage (..) f32; ns (..) u32) on
    the CPU, from the source the device kernel is compiled from -> uint8 (coverage's shape, 4).  No GPU needed."""
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    backdrop = np.ascontiguousarray(backdrop, dtype=np.float32)
    coverage = np.ascontiguousarray(coverage, dtype=np.float32)
    ns = np.ascontiguousarray(ns, dtype=np.uint32)
    n = coverage.size
    if not n or rgb.size != 3 * n or backdrop.size != 3 * n or ns.size != n:
        raise ValueError("rgb and backdrop hold 3 floats, coverage and ns one value per pixel of a frame that is not empty")
    out = np.zeros(coverage.shape + (4,), np.uint8)
    _check(lib().qa_test_matte_rgba_host(rgb.ctypes.data, backdrop.ctypes.data, coverage.ctypes.data, ns.ctypes.data, n, int(bool(srgb)), out.ctypes.data))
    return out


def _ao_keys(stream, c):
    """The (stream, counter) pairs of a hook call as two contiguous uint32 arrays of one length"""
    stream = np.ascontiguousarray(stream, dtype=np.uint32).reshape(-1)
    c = np.ascontiguousarray(c, dtype=np.uint32).reshape(-1)
    if c.shape != stream.shape:
        raise ValueError(f"c: shape {stream.shape} is expected, not {c.shape}")
    return stream, c


def _ao_vectors(name, v, count):
    """(count, 3) contiguous float32 from (count, 3), or from one vector for every record"""
    v = np.asarray(v, dtype=np.float32)
    if v.shape == (3,):
        v = np.broadcast_to(v, (count, 3))
    if v.shape != (count, 3):
        raise ValueError(f"{name}: shape ({count}, 3) or (3,) is expected, not {v.shape}")
    return np.ascontiguousarray(v)


def ao_directions_host(seed, stream, c, n):
    """qa_test_ao_directions_host: the ambient-occlusion directions of the keys (seed, stream[i], c[i]) about the unit normals n
    ((count, 3), or one (3,) for all) on the CPU, from the source the device kernels are compiled from -> float32 (count, 3).  No GPU
    needed."""
    stream, c = _ao_keys(stream, c)
    n = _ao_vectors("n", n, len(c))
    d = np.zeros((len(c), 3), np.float32)
    _check(lib().qa_test_ao_directions_host(int(seed) & 0xFFFFFFFF, stream.ctypes.data, c.ctypes.data, n.ctypes.data, len(c), d.ctypes.data))
    return d


def ao_face_normal_host(N, d):
    """qa_test_ao_face_normal_host: the normals N (count, 3) turned against the camera rays' directions d (count, 3) -> float32
    (count, 3).  No GPU needed."""
    N = np.ascontiguousarray(N, dtype=np.float32).reshape(-1, 3)
    d = _ao_vectors("d", d, len(N))
    out = np.zeros((len(N), 3), np.float32)
    _check(lib().qa_test_ao_face_normal_host(N.ctypes.data, d.ctypes.data, len(N), out.ctypes.data))
    return out


def ao_sphere_host(seed, stream, c):
    """qa_test_ao_sphere_host: the generator's inner step - the sphere points of the keys and whether all attempts failed -> (float32
    (count, 3), bool (count,)).  No GPU needed."""
    stream, c = _ao_keys(stream, c)
    s = np.zeros((len(c), 3), np.float32)
    fb = np.zeros(len(c), np.uint8)
    _check(lib().qa_test_ao_sphere_host(int(seed) & 0xFFFFFFFF, stream.ctypes.data, c.ctypes.data, len(c), s.ctypes.data, fb.ctypes.data))
    return s, fb.astype(bool)


def ao_direction_from_host(n, s):
    """qa_test_ao_direction_from_host: the generator's outer step from sphere points s (count, 3) given directly, about n ((count, 3) or
    (3,)) -> float32 (count, 3).  No GPU needed."""
    s = np.ascontiguousarray(s, dtype=np.float32).reshape(-1, 3)
    n = _ao_vectors("n", n, len(s))
    d = np.zeros((len(s), 3), np.float32)
    _check(lib().qa_test_ao_direction_from_host(n.ctypes.data, s.ctypes.data, len(s), d.ctypes.data))
    return d


def probe_directions_host(m, stream_ids=(0,), seed=DEFAULT_SEED, jitter=False):
    """qa_test_probe_directions_host: the K = 6 m^2 directions of a light probe's cube map, their weights (the texels' solid angles)
    and the random-number streams of their rays, for the probes with the given stream ids, on the CPU from the source the device
    kernels are compiled from -> (d float32 (n, K, 3), w float32 (n, K), ray_stream uint32 (n, K)).  No GPU needed."""
    s = np.ascontiguousarray(stream_ids, dtype=np.uint32).reshape(-1)
    m = int(m)
    if not 1 <= m <= QA_PROBE_MAX_M:
        raise ValueError(f"m: 1 .. {QA_PROBE_MAX_M} is expected, not {m}")
    K = 6 * m * m
    d, w, rs = np.zeros((len(s), K, 3), np.float32), np.zeros((len(s), K), np.float32), np.zeros((len(s), K), np.uint32)
    _check(lib().qa_test_probe_directions_host(m, int(seed) & 0xFFFFFFFF, QA_PROBE_JITTER if jitter else 0, s.ctypes.data, len(s), d.ctypes.data,
                                               w.ctypes.data, rs.ctypes.data))
    return d, w, rs


def probe_project_host(d, w, rgb, t):
    """qa_test_probe_project_host: one probe's K rays - directions d (K, 3), weights w (K,), radiance rgb (K, 3), hit parameters t
    (K,) - projected as a wave of the device kernel projects them -> (sh float32 (9, 3), hits int, tmin float32).  No GPU needed."""
    d = np.ascontiguousarray(d, dtype=np.float32).reshape(-1, 3)
    K = len(d)
    w, t = (np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in (w, t))
    rgb = np.ascontiguousarray(rgb, dtype=np.float32).reshape(-1, 3)
    if w.shape != (K,) or t.shape != (K,) or rgb.shape != (K, 3):
        raise ValueError(f"w, t: shape ({K},) and rgb: shape ({K}, 3) are expected, not {w.shape}, {t.shape}, {rgb.shape}")
    sh, hits, tmin = np.zeros((9, 3), np.float32), np.zeros(1, np.uint32), np.zeros(1, np.float32)
    _check(lib().qa_test_probe_project_host(K, d.ctypes.data, w.ctypes.data, rgb.ctypes.data, t.ctypes.data, sh.ctypes.data, hits.ctypes.data, tmin.ctypes.data))
    return sh, int(hits[0]), tmin[0]


def _probe_sh_array(sh):
    sh = np.ascontiguousarray(sh, dtype=np.float32)
    if sh.ndim < 2 or sh.shape[-2:] != (9, 3):
        raise ValueError(f"sh: shape (..., 9, 3) is expected, not {sh.shape}")
    return sh.reshape(-1, 9, 3)


def probe_shade_host(sh, normals, index=None):
    """qa_test_probe_shade_host: Context.probe_shade_device over host arrays - sh (probes, 9, 3), normals (n, 3), index (n,) int32 or
    None (shading point i takes probe i) -> rgb float32 (n, 3).  No GPU needed."""
    sh = _probe_sh_array(sh)
    nr = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
    n = len(nr)
    if index is not None:
        index = np.ascontiguousarray(index, dtype=np.int32)
        if index.shape != (n,):
            raise ValueError(f"index: shape ({n},) is expected, not {index.shape}")
    rgb = np.zeros((n, 3), np.float32)
    _check(lib().qa_test_probe_shade_host(n, sh.ctypes.data, len(sh), nr.ctypes.data, None if index is None else index.ctypes.data, rgb.ctypes.data))
    return rgb


def _probe_grid_args(origin, spacing, counts):
    """The three host arrays of a grid call"""
    o, sp = (np.ascontiguousarray(a, dtype=np.float32) for a in (origin, spacing))
    cn = np.ascontiguousarray(counts, dtype=np.int32)
    if o.shape != (3,) or sp.shape != (3,) or cn.shape != (3,):
        raise ValueError("origin, spacing and counts hold three values each")
    return o, sp, cn


def probe_grid_shade_host(sh, origin, spacing, counts, points, normals):
    """qa_test_probe_grid_shade_host: ProbeGrid.shade_device over host arrays - sh (nz * ny * nx, 9, 3) of the grid (origin, spacing,
    counts), points and normals (n, 3) -> rgb float32 (n, 3).  No GPU needed."""
    sh = _probe_sh_array(sh)
    o, sp, cn = _probe_grid_args(origin, spacing, counts)
    if (cn >= 1).all() and len(sh) != int(np.prod(cn.astype(np.int64))):
        raise ValueError(f"sh: {int(np.prod(cn.astype(np.int64)))} probes are expected, not {len(sh)}")
    p, nr, n = _ray_arrays(points, normals)
    rgb = np.zeros((n, 3), np.float32)
    _check(lib().qa_test_probe_grid_shade_host(n, sh.ctypes.data, o.ctypes.data, sp.ctypes.data, cn.ctypes.data, p.ctypes.data, nr.ctypes.data, rgb.ctypes.data))
    return rgb


def probevis_moments_host(t, m, d, dmax):
    """qa_test_probevis_moments_host: the hit parameters t (6 m^2,) of one probe's rays (probe_directions_host's order; a miss is
    QA_RAY_MISS) -> float32 (6, d, d, 2): per direction cell the mean of min(t, dmax) and of its square over the (m / d)^2 texels
    the cell pools.  No GPU needed."""
    m, d = int(m), int(d)
    t = np.ascontiguousarray(t, dtype=np.float32).reshape(-1)
    if not 1 <= m <= QA_PROBE_MAX_M or not 1 <= d <= m or m % d:
        raise ValueError(f"1 <= d <= m <= {QA_PROBE_MAX_M} with m % d == 0 is expected, not m {m}, d {d}")
    if t.shape != (6 * m * m,):
        raise ValueError(f"t: {6 * m * m} values are expected, not {t.shape}")
    out = np.zeros((6, d, d, 2), np.float32)
    _check(lib().qa_test_probevis_moments_host(m, d, float(dmax), t.ctypes.data, out.ctypes.data))
    return out


def _probevis_moments_array(moments, probes):
    mo = np.ascontiguousarray(moments, dtype=np.float32)
    if mo.ndim != 5 or mo.shape[1] != 6 or mo.shape[2] != mo.shape[3] or mo.shape[4] != 2 or not 1 <= mo.shape[2] <= QA_PROBE_MAX_M:
        raise ValueError(f"moments: shape (probes, 6, d, d, 2) is expected, not {mo.shape}")
    if len(mo) != probes:
        raise ValueError(f"moments: {probes} probes are expected, not {len(mo)}")
    return mo, int(mo.shape[2])


def probevis_grid_shade_host(sh, moments, origin, spacing, counts, points, normals, normal_bias=0.0):
    """qa_test_probevis_grid_shade_host: ProbeGrid.shade_device(visibility=True) over host arrays - sh (nz * ny * nx, 9, 3) and
    moments (nz * ny * nx, 6, d, d, 2) of the grid (origin, spacing, counts), points and normals (n, 3) -> rgb float32 (n, 3).  No
    GPU needed."""
    sh = _probe_sh_array(sh)
    o, sp, cn = _probe_grid_args(origin, spacing, counts)
    if (cn >= 1).all() and len(sh) != int(np.prod(cn.astype(np.int64))):
        raise ValueError(f"sh: {int(np.prod(cn.astype(np.int64)))} probes are expected, not {len(sh)}")
    mo, d = _probevis_moments_array(moments, len(sh))
    p, nr, n = _ray_arrays(points, normals)
    rgb = np.zeros((n, 3), np.float32)
    par = ProbeVisParams.of(d, None, normal_bias)
    _check(lib().qa_test_probevis_grid_shade_host(n, sh.ctypes.data, mo.ctypes.data, d, o.ctypes.data, sp.ctypes.data, cn.ctypes.data, p.ctypes.data,
                                                  nr.ctypes.data, C.byref(par), rgb.ctypes.data))
    return rgb


def reflprobe_layout(m, levels=None):
    """qa_reflprobe_layout: the chain of a reflection probe of m x m texels per face (a power of two in 1 .. 128) with `levels` levels
    (None: log2 m + 1, down to one texel per face) -> dict: levels, offset uint32 (levels,) the first texel of each level, res uint32
    (levels,) its texels per face edge m >> l, squarings uint32 (levels,) s with the level's Phong exponent 2^s (level 0 is the cube
    itself: 0 there), texels T of a probe's chain.  No GPU needed."""
    m = int(m)
    if m < 1 or m > QA_PROBE_MAX_M or m & (m - 1):
        raise ValueError(f"m: a power of two in 1 .. {QA_PROBE_MAX_M} is expected, not {m}")
    lg = m.bit_length() - 1
    levels = lg + 1 if levels is None else int(levels)
    if not 1 <= levels <= lg + 1:
        raise ValueError(f"levels: 1 .. {lg + 1} is expected for m = {m}, not {levels}")
    offset, res, sq = (np.zeros(levels, np.uint32) for _ in range(3))
    texels = C.c_uint64(0)
    _check(lib().qa_reflprobe_layout(m, levels, offset.ctypes.data, res.ctypes.data, sq.ctypes.data, C.addressof(texels)))
    return {"levels": levels, "offset": offset, "res": res, "squarings": sq, "texels": int(texels.value)}


def reflprobe_level(glossiness, m, levels=None):
    """The level of a chain at which a Blinn material of that glossiness looks: level l holds the Phong exponent 2^(2 (lg - l) - 1), and
    a Blinn exponent alpha is about the Phong exponent alpha / 4 around the mirror direction, so
    level = lg - (log2(glossiness / 4) + 1) / 2, clamped to [0, levels - 1] -> float32 array like glossiness.  An approximation for
    choosing the argument of reflprobe_shade_device, not part of its specification.  numpy, host only."""
    lay = reflprobe_layout(m, levels)
    lg = int(m).bit_length() - 1
    with np.errstate(all="ignore"):
        g = np.asarray(glossiness, np.float64)
        level = lg - (np.log2(g / 4.0) + 1.0) / 2.0
    return np.clip(np.nan_to_num(level, nan=0.0), 0.0, lay["levels"] - 1).astype(np.float32)


def _reflprobe_chain_array(chain, m, levels):
    """A host chain (probes, T, 3) checked against its layout -> (chain, levels)"""
    lay = reflprobe_layout(m, levels)
    chain = np.ascontiguousarray(chain, dtype=np.float32)
    if chain.ndim != 3 or chain.shape[1:] != (lay["texels"], 3):
        raise ValueError(f"chain: shape (probes, {lay['texels']}, 3) is expected, not {chain.shape}")
    return chain, lay["levels"]


def _reflprobe_lookup_arrays(dirs, level):
    d = np.ascontiguousarray(dirs, dtype=np.float32)
    n = _ray_count("dirs", d)
    lv = np.ascontiguousarray(np.broadcast_to(np.asarray(level, np.float32), (n,)))
    return d, lv, n


def reflprobe_prefilter_host(cube, levels=None):
    """qa_test_reflprobe_prefilter_host: Context.reflprobe_prefilter_device over a host array - cube (n, 6, m, m, 3) -> chain float32
    (n, T, 3).  No GPU needed."""
    cube = np.ascontiguousarray(cube, dtype=np.float32)
    if cube.ndim != 5 or cube.shape[1] != 6 or cube.shape[2] != cube.shape[3] or cube.shape[4] != 3:
        raise ValueError(f"cube: shape (n, 6, m, m, 3) is expected, not {cube.shape}")
    n, m = int(cube.shape[0]), int(cube.shape[2])
    lay = reflprobe_layout(m, levels)
    chain = np.zeros((n, lay["texels"], 3), np.float32)
    _check(lib().qa_test_reflprobe_prefilter_host(n, cube.ctypes.data, m, lay["levels"], chain.ctypes.data))
    return chain


def reflprobe_shade_host(chain, m, dirs, level, levels=None, index=None):
    """qa_test_reflprobe_shade_host: Context.reflprobe_shade_device over host arrays - chain (probes, T, 3), dirs (n, 3), level (n,) or a
    number, index (n,) int32 or None (lookup i takes probe i) -> rgb float32 (n, 3).  No GPU needed."""
    chain, levels = _reflprobe_chain_array(chain, m, levels)
    d, lv, n = _reflprobe_lookup_arrays(dirs, level)
    if index is not None:
        index = np.ascontiguousarray(index, dtype=np.int32)
        if index.shape != (n,):
            raise ValueError(f"index: shape ({n},) is expected, not {index.shape}")
    rgb = np.zeros((n, 3), np.float32)
    _check(lib().qa_test_reflprobe_shade_host(n, chain.ctypes.data, len(chain), int(m), levels, d.ctypes.data, lv.ctypes.data, _ptr(index), rgb.ctypes.data))
    return rgb


def reflprobe_grid_shade_host(chain, m, origin, spacing, counts, points, dirs, level, levels=None):
    """qa_test_reflprobe_grid_shade_host: ProbeGrid.reflect_device over host arrays - chain (nz * ny * nx, T, 3) of the grid (origin,
    spacing, counts), points and dirs (n, 3), level (n,) or a number -> rgb float32 (n, 3).  No GPU needed."""
    chain, levels = _reflprobe_chain_array(chain, m, levels)
    o, sp, cn = _probe_grid_args(origin, spacing, counts)
    if (cn >= 1).all() and len(chain) != int(np.prod(cn.astype(np.int64))):
        raise ValueError(f"chain: {int(np.prod(cn.astype(np.int64)))} probes are expected, not {len(chain)}")
    p, d, n = _ray_arrays(points, dirs)
    lv = np.ascontiguousarray(np.broadcast_to(np.asarray(level, np.float32), (n,)))
    rgb = np.zeros((n, 3), np.float32)
    _check(lib().qa_test_reflprobe_grid_shade_host(n, chain.ctypes.data, int(m), levels, o.ctypes.data, sp.ctypes.data, cn.ctypes.data, p.ctypes.data,
                                                   d.ctypes.data, lv.ctypes.data, rgb.ctypes.data))
    return rgb


def _bake_size(width, height):
    """(width, height) of a bake call as the C ABI takes them; the library refuses 0 and above QA_BAKE_MAX_DIM, a negative one is
    refused here (it would wrap)"""
    w, h = int(width), int(height)
    if w < 0 or h < 0 or w > 0xFFFFFFFF or h > 0xFFFFFFFF:
        raise ValueError(f"width, height: {w} x {h} texels")
    return w, h


def _bake_host_planes(w, h, want):
    """The numpy planes of a host bake call: those named in `want` (all of BAKE_PLANES when it is None)"""
    names = BAKE_PLANES if want is None else tuple(want)
    bad = [k for k in names if k not in BAKE_PLANES]
    if bad:
        raise ValueError(f"planes: {bad} are not among {BAKE_PLANES}")
    shapes = {"point": (h, w, 3), "normal": (h, w, 3), "face": (h, w), "bary": (h, w, 2)}
    return {k: np.zeros(shapes[k], np.int32 if k == "face" else np.float32) for k in BAKE_PLANES if k in names}


def bake_texels_host(blob, node, width, height, texmap=None, mtl=-1, planes=None):
    """qa_test_bake_texels_host: Context.bake_texels on a flat scene blob (numpy uint8) on the CPU, from the source the device kernel
    is compiled from (the opening comment of qa_bake_dev.h is the specification), every refusal but the missing scene's included
    -> dict of numpy arrays point [h,w,3] f32, normal [h,w,3] f32, face [h,w] i32, bary [h,w,2] f32 (planes: the names wanted; None:
    all four).  No GPU needed."""
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    w, h = _bake_size(width, height)
    out = _bake_host_planes(w, h, planes)
    _check(lib().qa_test_bake_texels_host(blob.ctypes.data, blob.size, int(node), -1 if texmap is None else int(texmap), int(mtl), w, h,
                                          *(out[k].ctypes.data if k in out else None for k in BAKE_PLANES)))
    return out


def _dilate_arrays(rgb8, face):
    rgb8 = np.ascontiguousarray(rgb8)
    face = np.ascontiguousarray(face)
    if rgb8.dtype != np.uint8 or rgb8.ndim != 3 or rgb8.shape[2] != 3:
        raise ValueError("rgb8: a uint8 array of shape (h, w, 3) is expected")
    if face.dtype != np.int32 or face.shape != rgb8.shape[:2]:
        raise ValueError(f"face: an int32 array of shape {rgb8.shape[:2]} is expected")
    return rgb8, face


def bake_dilate_host(rgb8, face, radius=2, out=None):
    """qa_test_bake_dilate_host: Context.bake_dilate_device over numpy arrays on the CPU, from the source the device kernel is compiled
    from: rgb8 (h, w, 3) uint8, face (h, w) int32 -> uint8 (h, w, 3) (out: the array to write; it must not be rgb8).  No GPU needed."""
    rgb8, face = _dilate_arrays(rgb8, face)
    if out is None:
        out = np.zeros_like(rgb8)
    if not isinstance(out, np.ndarray) or out.dtype != np.uint8 or out.shape != rgb8.shape or not out.flags.c_contiguous:
        raise ValueError(f"out: a contiguous uint8 array of shape {rgb8.shape} is expected")
    h, w = face.shape
    _check(lib().qa_test_bake_dilate_host(rgb8.ctypes.data, face.ctypes.data, w, h, int(radius), out.ctypes.data))
    return out


def _idmatte_key(key):
    """The C ABI's key of "node" / "material" (or of the constant itself)"""
    if key in _IDMATTE_KEYS:
        return _IDMATTE_KEYS[key]
    if key in _IDMATTE_KEYS.values():
        return int(key)
    raise ValueError(f"key: 'node' or 'material' is expected, not {key!r}")


def _idmatte_select_list(select):
    """The id list of a select call as a contiguous int32 array of at most QA_IDMATTE_MAX_SELECT entries"""
    sel = np.ascontiguousarray(np.asarray(select, dtype=np.int64).reshape(-1))
    if sel.size > QA_IDMATTE_MAX_SELECT:
        raise ValueError(f"select: at most {QA_IDMATTE_MAX_SELECT} ids, not {sel.size}")
    if sel.size and (sel.min() < -2 ** 31 or sel.max() > 2 ** 31 - 1):
        raise ValueError("select: ids are int32")
    return sel.astype(np.int32)


def idmatte_accumulate_host(hit, keys):
    """qa_test_idmatte_accumulate_host: one pixel's ranked id table from its n samples on the CPU, from the source the device kernel
    is compiled from.  hit (n,) bool; keys (n,) int32, read where hit is set -> dict ids (8,) i32, counts (8,) u32, other () u32.
    No GPU needed."""
    hit = np.ascontiguousarray(hit).astype(np.uint8).reshape(-1)
    keys = np.ascontiguousarray(keys, dtype=np.int32).reshape(-1)
    if keys.shape != hit.shape:
        raise ValueError(f"keys: shape {hit.shape} is expected, not {keys.shape}")
    out = {"ids": np.zeros(QA_IDMATTE_SLOTS, np.int32), "counts": np.zeros(QA_IDMATTE_SLOTS, np.uint32), "other": np.zeros(1, np.uint32)}
    _check(lib().qa_test_idmatte_accumulate_host(hit.ctypes.data, keys.ctypes.data, len(hit), out["ids"].ctypes.data, out["counts"].ctypes.data,
                                                 out["other"].ctypes.data))
    out["other"] = out["other"].reshape(())
    return out


def idmatte_select_host(ids, counts, samples, select):
    """qa_test_idmatte_select_host: the coverage of the ids of `select` (at most QA_IDMATTE_MAX_SELECT) from an id matte's planes (ids
    (.., 8) i32, counts (.., 8) u32, samples (..) u32) on the CPU, from the source the device kernel is compiled from -> float32 of
    samples' shape.  No GPU needed."""
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    samples = np.ascontiguousarray(samples, dtype=np.uint32)
    n = samples.size
    if not n or ids.shape != samples.shape + (QA_IDMATTE_SLOTS,) or counts.shape != ids.shape:
        raise ValueError("ids and counts hold 8 values, samples one per pixel of a frame that is not empty")
    sel = _idmatte_select_list(select)
    out = np.zeros(samples.shape, np.float32)
    _check(lib().qa_test_idmatte_select_host(ids.ctypes.data, counts.ctypes.data, samples.ctypes.data, n, sel.ctypes.data if sel.size else None,
                                             sel.size, out.ctypes.data))
    return out


def _denoise_flags(normal, albedo, variance):
    """The flag word of a denoise call: the planes that are given."""
    return ((QA_DENOISE_GUIDE_NORMAL if normal is not None else 0) | (QA_DENOISE_GUIDE_ALBEDO if albedo is not None else 0)
            | (QA_DENOISE_GUIDE_VARIANCE if variance is not None else 0))


def _denoise_host_planes(rgb, depth, ns, normal=None, albedo=None, variance=None):
    """What the three denoise*_host calls share: the planes as contiguous arrays of their types, their shapes checked, and a new
    output -> ((h, w), the pointers of the six planes in the C ABI's order (None for a plane that is not given), keep, out, flags):
    keep, the arrays behind the pointers, for the caller to hold until the call has returned; flags, the planes given."""
    keep = [np.ascontiguousarray(rgb, dtype=np.float32), np.ascontiguousarray(depth, dtype=np.float32), np.ascontiguousarray(ns, dtype=np.uint32)]
    keep += [None if g is None else np.ascontiguousarray(g, dtype=np.float32) for g in (normal, albedo, variance)]
    rgb, depth, ns, *guides = keep
    assert rgb.ndim == 3 and rgb.shape[2] == 3 and depth.shape == rgb.shape[:2] and ns.shape == rgb.shape[:2]
    assert all(g is None or g.shape == rgb.shape for g in guides[:2]) and (guides[2] is None or guides[2].shape == depth.shape)
    return depth.shape, [_ptr(a) for a in keep], keep, np.zeros(rgb.shape, np.float32), _denoise_flags(normal, albedo, variance)


def denoise_host(rgb, depth, ns, params=None, iterations=None, sigma_color=None, sigma_depth=None):
    """qa_test_denoise_host: the edge-avoiding filter of Context.denoise_device on the CPU, from the source the device kernels are
    compiled from: rgb (h, w, 3), depth (h, w), ns (h, w) -> float32 (h, w, 3).  The inputs are not modified.  No GPU needed."""
    (h, w), ptrs, keep, out, _ = _denoise_host_planes(rgb, depth, ns)
    p = DenoiseParams.of(params, iterations, sigma_color, sigma_depth)
    _check(lib().qa_test_denoise_host(*ptrs[:3], w, h, C.byref(p), out.ctypes.data))
    return out


def denoise_guided_host(rgb, depth, ns, normal=None, albedo=None, params=None, iterations=None, sigma_color=None, sigma_depth=None,
                        sigma_normal=None):
    """qa_test_denoise_guided_host: the guided filter of Context.denoise_guided_device on the CPU, from the source the device kernels
    are compiled from; normal / albedo (h, w, 3) or None: the flags are the guides given.  -> float32 (h, w, 3).  No GPU needed."""
    (h, w), ptrs, keep, out, flags = _denoise_host_planes(rgb, depth, ns, normal, albedo)
    p = DenoiseGuidedParams.of(params, flags, iterations, sigma_color, sigma_depth, sigma_normal)
    _check(lib().qa_test_denoise_guided_host(*ptrs[:5], w, h, C.byref(p), out.ctypes.data))
    return out


def denoise_variance_host(rgb, depth, ns, normal=None, albedo=None, variance=None, params=None, iterations=None, sigma_color=None,
                          sigma_depth=None, sigma_normal=None, variance_scale=None):
    """qa_test_denoise_variance_host: Context.denoise_variance_device on the CPU, from the source the device kernels are compiled
    from; normal / albedo (h, w, 3) and variance (h, w) or None: the flags are the planes given.  -> float32 (h, w, 3).  No GPU needed."""
    (h, w), ptrs, keep, out, flags = _denoise_host_planes(rgb, depth, ns, normal, albedo, variance)
    p = DenoiseVarianceParams.of(params, flags, iterations, sigma_color, sigma_depth, sigma_normal, variance_scale)
    _check(lib().qa_test_denoise_variance_host(*ptrs, w, h, C.byref(p), out.ctypes.data))
    return out


def _denoise_device_planes(rgb, depth, ns, out, normal=None, albedo=None, variance=None):
    """What the three Context.denoise*_device calls share: the torch planes checked (float32 [h,w,3], float32 [h,w], int32/uint32
    [h,w]; the guides float32 [h,w,3], the variance float32 [h,w], or None) and out checked, or allocated where it is None
    -> ((h, w), the pointers of the six planes in the C ABI's order (None for a plane that is not given), out, flags: the planes given)."""
    import torch
    assert rgb.is_cuda and rgb.is_contiguous() and rgb.dim() == 3 and rgb.shape[2] == 3 and rgb.dtype == torch.float32
    h, w = rgb.shape[:2]
    n = h * w
    assert depth.is_cuda and depth.is_contiguous() and depth.numel() == n and depth.element_size() == 4
    assert ns.is_cuda and ns.is_contiguous() and ns.numel() == n and ns.element_size() == 4
    for g, k in ((normal, 3), (albedo, 3), (variance, 1)):
        assert g is None or (g.is_cuda and g.is_contiguous() and g.numel() == k * n and g.dtype == torch.float32)
    if out is None:
        out = torch.empty_like(rgb)
    assert out.is_cuda and out.is_contiguous() and out.shape == rgb.shape and out.dtype == torch.float32
    return (h, w), [_ptr(t) for t in (rgb, depth, ns, normal, albedo, variance)], out, _denoise_flags(normal, albedo, variance)


def _camera_record(cam):
    """A camera (a record of CAMERA_DTYPE: host.HostScene.camera(), blob_camera(blob)) as a contiguous array of one record of its own."""
    return np.array(cam, dtype=CAMERA_DTYPE).reshape(1)


def _ptr(a):
    """The address of a numpy array or a torch tensor for a ctypes call; None stays None."""
    return None if a is None else a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()


def _reproject_host_planes(cur, history, prev_cam, cur_cam, origin, ids, hist_ids, out, out_length):
    """What the three reproject*_host calls share: the planes as contiguous arrays of their types and shapes, out / out_length
    allocated where they are not given -> ((h, w), head, keep, out, out_length): head, the C call's arguments from prev_cam to
    hist_ids; keep, the arrays behind its pointers, for the caller to hold until the call has returned."""
    rgb, depth, ns = cur
    rgb = rgb if out is rgb and rgb is not None else np.ascontiguousarray(rgb, dtype=np.float32)
    depth = np.ascontiguousarray(depth, dtype=np.float32)
    ns = np.ascontiguousarray(ns, dtype=np.uint32)
    assert rgb.ndim == 3 and rgb.shape[2] == 3 and depth.shape == rgb.shape[:2] and ns.shape == rgb.shape[:2]
    h, w = depth.shape
    hist = [np.ascontiguousarray(a, dtype=np.float32) for a in history]
    assert hist[0].shape == (h, w, 3) and hist[1].shape == (h, w) and hist[2].shape == (h, w)
    idp = [None if a is None else np.ascontiguousarray(a, dtype=np.int32) for a in (ids, hist_ids)]
    assert all(a is None or a.shape == (h, w, 2) for a in idp)
    out = np.zeros((h, w, 3), np.float32) if out is None else out
    out_length = np.zeros((h, w), np.float32) if out_length is None else out_length
    for a, shape in ((out, (h, w, 3)), (out_length, (h, w))):
        assert a.dtype == np.float32 and a.flags.c_contiguous and a.shape == shape
    keep = [_camera_record(prev_cam), _camera_record(cur_cam), rgb, depth, ns, idp[0], *hist, idp[1]]
    head = [_ptr(keep[0]), _ptr(keep[1]), int(origin[0]), int(origin[1]), w, h, *(_ptr(a) for a in keep[2:])]
    return (h, w), head, keep, out, out_length


def _reproject_history_tensors(h, w, device, history, hist_ids, out, out_length):
    """The history and the outputs of a device reprojection, checked: float32 CUDA tensors [h,w,3], [h,w], [h,w], hist_ids int32
    [h,w,2] or None; out / out_length allocated where they are not given -> (the four history pointers, out, out_length)."""
    import torch
    n = h * w
    hrgb, hdepth, hlen = history
    for t, k in ((hrgb, 3), (hdepth, 1), (hlen, 1)):
        assert t.is_cuda and t.is_contiguous() and t.numel() == k * n and t.dtype == torch.float32
    assert hist_ids is None or (hist_ids.is_cuda and hist_ids.is_contiguous() and hist_ids.numel() == 2 * n and hist_ids.dtype == torch.int32)
    if out is None:
        out = torch.empty((h, w, 3), dtype=torch.float32, device=device)
    if out_length is None:
        out_length = torch.empty((h, w), dtype=torch.float32, device=device)
    assert out.is_cuda and out.is_contiguous() and out.numel() == 3 * n and out.dtype == torch.float32
    assert out_length.is_cuda and out_length.is_contiguous() and out_length.numel() == n and out_length.dtype == torch.float32
    return [_ptr(hrgb), _ptr(hdepth), _ptr(hlen), _ptr(hist_ids)], out, out_length


def _reproject_device_planes(cur, history, prev_cam, cur_cam, origin, ids, hist_ids, out, out_length):
    """What the three Context.reproject*_device calls share: the torch planes checked, out / out_length allocated where they are
    not given -> ((h, w), head, keep, out, out_length): head, the C call's arguments from prev_cam to hist_ids; keep, the camera
    records behind its first two pointers."""
    import torch
    rgb, depth, ns = cur
    assert rgb.is_cuda and rgb.is_contiguous() and rgb.dim() == 3 and rgb.shape[2] == 3 and rgb.dtype == torch.float32
    h, w = rgb.shape[:2]
    for t in (depth, ns):
        assert t.is_cuda and t.is_contiguous() and t.numel() == h * w and t.element_size() == 4
    assert depth.dtype == torch.float32
    assert ids is None or (ids.is_cuda and ids.is_contiguous() and ids.numel() == 2 * h * w and ids.dtype == torch.int32)
    hist, out, out_length = _reproject_history_tensors(h, w, rgb.device, history, hist_ids, out, out_length)
    keep = [_camera_record(prev_cam), _camera_record(cur_cam)]
    head = [_ptr(keep[0]), _ptr(keep[1]), int(origin[0]), int(origin[1]), w, h, _ptr(rgb), _ptr(depth), _ptr(ns), _ptr(ids), *hist]
    return (h, w), head, keep, out, out_length


def _reproject_progressive_planes(frame, history, prev_cam, hist_ids, out, out_length):
    """What the three Progressive.reproject*_device calls share (the current planes and the region are the frame's own)
    -> ((h, w), device, head, keep, out, out_length): head, the C call's arguments from the context to hist_ids; keep, the camera
    record behind its pointer."""
    import torch
    device = torch.device("cuda", frame._ctx.device_id)
    x0, y0, x1, y1 = frame.region
    h, w = y1 - y0, x1 - x0
    hist, out, out_length = _reproject_history_tensors(h, w, device, history, hist_ids, out, out_length)
    keep = _camera_record(prev_cam)
    return (h, w), device, [frame._ctx._h, _ptr(keep), *hist], keep, out, out_length


def reproject_host(cur, history, prev_cam, cur_cam, origin=(0, 0), ids=None, hist_ids=None, out=None, out_length=None, params=None,
                   depth_tolerance=None, max_history=None):
    """qa_test_reproject_host: the temporal reprojection of Context.reproject_device on the CPU, from the source the device kernel is
    compiled from.  cur = (rgb (h, w, 3) f32, depth (h, w) f32, ns (h, w) u32) rendered from cur_cam; history = (rgb, depth,
    length (h, w) f32) accumulated under prev_cam; origin: the image pixel (x0, y0) of the frames' first pixel; ids / hist_ids:
    (h, w, 2) i32, both or neither.  out / out_length: float32 arrays to write (out may be cur's rgb itself) -> (out (h, w, 3),
    out_length (h, w)).  The other inputs are not modified.  No GPU needed."""
    _, head, keep, out, out_length = _reproject_host_planes(cur, history, prev_cam, cur_cam, origin, ids, hist_ids, out, out_length)
    p = ReprojectParams.of(params, depth_tolerance, max_history)
    _check(lib().qa_test_reproject_host(*head, C.byref(p), _ptr(out), _ptr(out_length)))
    return out, out_length


def node_motion(prev_instances, cur_instances):
    """qa_reproject_node_motion: the motion table (NODE_MOTION_DTYPE, one record per node) between two states of one scene graph,
    each the whole INSTANCE_DTYPE table (blob_table(blob, "instances"), or an edited copy of it): record k takes a world point of
    the current scene to where the same point of node k lay in the previous one; moved = 0 and the exact identity where the node
    and all its ancestors stand as they stood.  No GPU needed."""
    prev = np.ascontiguousarray(prev_instances, dtype=INSTANCE_DTYPE).reshape(-1)
    cur = np.ascontiguousarray(cur_instances, dtype=INSTANCE_DTYPE).reshape(-1)
    assert prev.shape == cur.shape, "two tables of one scene"
    out = np.zeros(len(cur), NODE_MOTION_DTYPE)
    _check(lib().qa_reproject_node_motion(prev.ctypes.data, cur.ctypes.data, len(cur), out.ctypes.data))
    return out


def reproject_motion_host(cur, history, prev_cam, cur_cam, origin=(0, 0), ids=None, hist_ids=None, motion=None, out=None, out_length=None,
                          params=None, depth_tolerance=None, max_history=None, clamp=None, clamp_radius=None, clamp_gamma=None):
    """qa_test_reproject_motion_host: Context.reproject_motion_device on the CPU, from the source the device kernel is compiled
    from; the arguments of reproject_host, and motion: a table of NODE_MOTION_DTYPE (node_motion()) - given, it sets
    QA_REPROJECT_MOTION; clamp (bool) sets or clears QA_REPROJECT_CLAMP, clamp_radius / clamp_gamma override params' values.
    -> (out (h, w, 3), out_length (h, w)).  No GPU needed."""
    _, head, keep, out, out_length = _reproject_host_planes(cur, history, prev_cam, cur_cam, origin, ids, hist_ids, out, out_length)
    table = None if motion is None else np.ascontiguousarray(motion, dtype=NODE_MOTION_DTYPE).reshape(-1)
    p = ReprojectMotionParams.of(params, depth_tolerance, max_history, True if table is not None else None, clamp, clamp_radius, clamp_gamma)
    _check(lib().qa_test_reproject_motion_host(*head, _ptr(table), 0 if table is None else len(table), C.byref(p), _ptr(out), _ptr(out_length)))
    return out, out_length


def reproject_moments_host(cur, history, prev_cam, cur_cam, origin=(0, 0), ids=None, hist_ids=None, hist_moments=None, motion=None, out=None,
                           out_length=None, out_moments=None, out_variance=None, params=None, depth_tolerance=None, max_history=None, clamp=None,
                           clamp_radius=None, clamp_gamma=None, moments=None, shorten=None, min_frames=None, shorten_rate=None):
    """qa_test_reproject_moments_host: Context.reproject_moments_device on the CPU, from the source the device kernel is compiled
    from; the arguments of reproject_motion_host, and hist_moments: (h, w, 2) f32 or None (nobody has moment history); moments /
    shorten (bool) set or clear QA_REPROJECT_MOMENTS / QA_REPROJECT_SHORTEN, min_frames / shorten_rate override params' values (a
    ReprojectMomentsParams).  -> (out (h, w, 3), out_length (h, w), out_moments (h, w, 2), out_variance (h, w)); the last two are
    None when QA_REPROJECT_MOMENTS is clear and they were not given.  No GPU needed."""
    (h, w), head, keep, out, out_length = _reproject_host_planes(cur, history, prev_cam, cur_cam, origin, ids, hist_ids, out, out_length)
    hmom = None if hist_moments is None else np.ascontiguousarray(hist_moments, dtype=np.float32)
    assert hmom is None or hmom.shape == (h, w, 2)
    table = None if motion is None else np.ascontiguousarray(motion, dtype=NODE_MOTION_DTYPE).reshape(-1)
    p = ReprojectMomentsParams.of(params, depth_tolerance, max_history, True if table is not None else None, clamp, clamp_radius, clamp_gamma, moments,
                                  shorten, min_frames, shorten_rate)
    if p.flags & QA_REPROJECT_MOMENTS:
        out_moments = np.zeros((h, w, 2), np.float32) if out_moments is None else out_moments
        out_variance = np.zeros((h, w), np.float32) if out_variance is None else out_variance
    for a, shape in ((out_moments, (h, w, 2)), (out_variance, (h, w))):
        assert a is None or (a.dtype == np.float32 and a.flags.c_contiguous and a.shape == shape)
    _check(lib().qa_test_reproject_moments_host(*head, _ptr(hmom), _ptr(table), 0 if table is None else len(table), C.byref(p), _ptr(out),
                                                _ptr(out_length), _ptr(out_moments), _ptr(out_variance)))
    return out, out_length, out_moments, out_variance


def _moments_tensors(p, h, w, device, hist_moments, out_moments, out_variance):
    """The moment planes of a device call checked, and with QA_REPROJECT_MOMENTS the two outputs allocated where they are not given."""
    import torch
    n = h * w
    if p.flags & QA_REPROJECT_MOMENTS:
        if out_moments is None:
            out_moments = torch.empty((h, w, 2), dtype=torch.float32, device=device)
        if out_variance is None:
            out_variance = torch.empty((h, w), dtype=torch.float32, device=device)
    for t, k in ((hist_moments, 2), (out_moments, 2), (out_variance, 1)):
        assert t is None or (t.is_cuda and t.is_contiguous() and t.numel() == k * n and t.dtype == torch.float32)
    return out_moments, out_variance


def _motion_tensor(motion, device, stream):
    """A motion table for a device call: a CUDA tensor of 64-byte records as it is, a numpy table of NODE_MOTION_DTYPE uploaded on
    the call's stream (None: torch's current one, which the call waits for) -> (tensor or None, records)."""
    import torch
    if motion is None:
        return None, 0
    if isinstance(motion, torch.Tensor):
        nbytes = motion.numel() * motion.element_size()
        assert motion.is_cuda and motion.is_contiguous() and nbytes and nbytes % 64 == 0
        return motion, nbytes // 64
    table = np.ascontiguousarray(motion, dtype=NODE_MOTION_DTYPE).reshape(-1)
    ts = torch.cuda.ExternalStream(stream, device=device) if stream else torch.cuda.current_stream(device)
    with torch.cuda.stream(ts):
        t = torch.from_numpy(table.view(np.uint8)).to(device)
    return t, len(table)


def _ray_tensor(name, t, shape, dtype, device):
    """A tensor of a ray-query call, checked before anything reaches the library: a contiguous torch tensor of that shape and dtype on
    the context's device."""
    import torch
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: a torch tensor is expected, not {type(t).__name__}")
    if t.device != device:
        raise ValueError(f"{name}: the tensor is on {t.device}, the context on {device}")
    if t.dtype != dtype:
        raise TypeError(f"{name}: dtype {dtype} is expected, not {t.dtype}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: shape {tuple(shape)} is expected, not {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: the tensor is not contiguous")
    return t


def _output_tensors(names, shapes, dtypes, device, given):
    """The output tensors of a device call: the ones given are written; when none is given all of `names` are allocated.  Each is
    checked as _ray_tensor checks -> (dict name -> tensor, pointers in the order of `names`: None for one that is not written)."""
    import torch
    out = {k: v for k, v in given.items() if v is not None}
    if not out:
        out = {k: torch.empty(shapes[k], dtype=dtypes[k], device=device) for k in names}
    for k, t in out.items():
        _ray_tensor(k, t, shapes[k], dtypes[k], device)
    return out, [out[k].data_ptr() if k in out else None for k in names]


def _region_planes(region, names):
    """Shapes and dtypes of the guide and matte planes of a region: coverage and depth one float per pixel, ids two int32, the rest
    three floats."""
    import torch
    x0, y0, x1, y1 = region
    h, w = y1 - y0, x1 - x0
    shapes = {k: (h, w) if k in ("coverage", "depth") else (h, w, 2) if k == "ids" else (h, w, 3) for k in names}
    return shapes, {k: torch.int32 if k == "ids" else torch.float32 for k in names}


def _idmatte_planes(region):
    """Shapes and dtypes of the id matte's planes of a region.  (torch has no uint32 worth the name: the unsigned planes are int32
    tensors of the same bits; no count reaches 2^31)"""
    import torch
    x0, y0, x1, y1 = region
    h, w = y1 - y0, x1 - x0
    shapes = {k: (h, w, QA_IDMATTE_SLOTS) if k in ("ids", "counts") else (h, w) for k in IDMATTE_PLANES}
    return shapes, {k: torch.int32 for k in IDMATTE_PLANES}


def _ao_planes(region):
    """Shapes and dtypes of the ambient-occlusion planes of a region (the unsigned planes are int32 tensors of the same bits, as the
    id matte's)"""
    import torch
    x0, y0, x1, y1 = region
    h, w = y1 - y0, x1 - x0
    return {k: (h, w) for k in AO_PLANES}, {k: torch.float32 if k == "ao" else torch.int32 for k in AO_PLANES}


def _ray_count(name, t):
    """n of an [n, 3] ray array (torch or numpy)"""
    if t.ndim != 2 or t.shape[1] != 3:
        raise ValueError(f"{name}: shape (n, 3) is expected, not {tuple(t.shape)}")
    if t.shape[0] > QA_MAX_RAYS:
        raise ValueError(f"{name}: more than 2^31 - 1 rays")
    return int(t.shape[0])


def _ray_arrays(origins, dirs):
    """The rays of a host call as two contiguous float32 [n, 3] arrays (anything numpy can make one of is converted)"""
    o, d = (np.ascontiguousarray(a, dtype=np.float32) for a in (origins, dirs))
    n = _ray_count("origins", o)
    if d.shape != o.shape:
        raise ValueError(f"dirs: shape {o.shape} is expected, not {d.shape}")
    return o, d, n


def _radiance_shape(name, t, spp):
    """(n, per_sample) of the origins of a radiance call: [n, 3], or [n, spp, 3] for rays per sample (torch or numpy)"""
    if t.ndim == 3 and t.shape[1] == spp and t.shape[2] == 3:
        n, per_sample = int(t.shape[0]), True
    elif t.ndim == 2 and t.shape[1] == 3:
        n, per_sample = int(t.shape[0]), False
    else:
        raise ValueError(f"{name}: shape (n, 3) or (n, {spp}, 3) is expected, not {tuple(t.shape)}")
    if n > QA_MAX_RAYS:
        raise ValueError(f"{name}: more than 2^31 - 1 rays")
    return n, per_sample


CAMERA_SAMPLE_OUTPUTS = ("origins", "dirs", "dx", "dy", "screen", "stream_ids")   # in the C ABI's order


def pick(ctx, x, y, seed=DEFAULT_SEED):
    """What pixel (x, y) sees -> (node, material, depth) of its first hit (node -1 on a miss); a one-pixel Context.gbuffer."""
    g = ctx.gbuffer((x, y, x + 1, y + 1), seed)
    return int(g["ids"][0, 0, 0]), int(g["ids"][0, 0, 1]), float(g["depth"][0, 0])


def texels_host(rgb8):
    """qa_test_texels_host: the float texel table's entries of an (h, w, 3) uint8 image (rows may be strided) on the CPU, from the
    source an upload and the texel-edit kernel are compiled from -> float32 (h, w, 4).  No GPU needed."""
    rgb8 = _rgb8_rows(rgb8)
    h, w = rgb8.shape[:2]
    out = np.zeros((h, w, 4), np.float32)
    _check(lib().qa_test_texels_host(rgb8.ctypes.data, w, h, rgb8.strides[0], out.ctypes.data))
    return out


def _rgb8_rows(a):
    """An (h, w, 3) uint8 numpy array whose rows are contiguous (a row stride is kept; anything else is copied)."""
    assert a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] == 3 and a.shape[0] > 0 and a.shape[1] > 0, "rgb8 must be (h, w, 3) uint8"
    if a.strides[2] != 1 or a.strides[1] != 3 or a.strides[0] < 3 * a.shape[1]:
        a = np.ascontiguousarray(a)
    return a


def _display_outputs(n, device, want, given):
    """The device outputs of a display call: names in `want` are allocated (torch uint8; stats: 4 words), `given` overrides;
    -> (dict name -> tensor or None, list of pointers in the C ABI's order)."""
    import torch
    out = {}
    for name in ("color", "count", "zimg", "countimg", "mask", "stats"):
        t = given.get(name)
        if t is None and name in want:
            t = torch.empty(4, dtype=torch.int32, device=device) if name == "stats" else \
                torch.empty(3 * n if name == "color" else n, dtype=torch.uint8, device=device)
        if t is not None:
            assert t.is_cuda and t.is_contiguous() and t.numel() * t.element_size() == (16 if name == "stats" else 3 * n if name == "color" else n)
        out[name] = t
    return out, [out[k].data_ptr() if out[k] is not None else None for k in ("color", "count", "zimg", "countimg", "mask", "stats")]


DISPLAY_ALL = ("color", "count", "zimg", "countimg", "mask", "stats")


def stats_from_tensor(t):
    """The statistics a display call wrote to the device (4 words) -> dict(zmin, zmax, smin, smax)."""
    a = t.cpu().numpy().view(DISPLAY_STATS_DTYPE)[0]
    return {k: a[k].item() for k in DISPLAY_STATS_DTYPE.names}


def strip_count(y0, y1, first_strip, strip_step):
    return int(lib().qa_strip_count(y0, y1, first_strip, strip_step))


class Context:
    """One integrator context = one GPU (the reference's Renderer instance on one MPI rank)."""

    def __init__(self, device_id=0):
        self._h = C.c_void_p()
        _check(lib().qa_ctx_create(int(device_id), C.byref(self._h)))
        self.device_id = int(device_id)
        self.size = None
        self._photon_sizes = None
        self._tmax_fill = None   # occluded_device: the tensor a scalar tmax was broadcast into, kept until the next such call
        self._bake_stream = None   # bake_ao: its side stream of torch's, made on first use, dropped by close()

    # -- scene ---------------------------------------------------------------------------------
    def upload_scene(self, blob):
        """blob: numpy uint8 array (host) holding a flat scene."""
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        _check(lib().qa_scene_upload(self._h, blob.ctypes.data, blob.size))
        self._remember_size(blob)
        self._photon_sizes = None   # a new scene drops the photon maps

    def upload_scene_device(self, dev_tensor):
        """dev_tensor: torch uint8 CUDA tensor holding a flat scene (e.g. after a broadcast)."""
        assert dev_tensor.is_cuda and dev_tensor.is_contiguous()
        _check(lib().qa_scene_upload_device(self._h, dev_tensor.data_ptr(), dev_tensor.numel()))
        self._remember_size(dev_tensor[:256].cpu().numpy())
        self._photon_sizes = None   # a new scene drops the photon maps

    def _remember_size(self, blob_head):
        # qa_flat_header: width/height follow magic,version(8) total_bytes(8) 6 vec3 (72) dof (4)
        w, h = np.frombuffer(bytes(bytearray(blob_head[92:100])), dtype=np.uint32)
        self.size = (int(w), int(h))

    # -- scene edits (qa_scene_edit_*): the context ends up as after upload_scene(edited blob), without a mesh rebuild ---------
    def edit_camera(self, cam):
        """cam: a record of CAMERA_DTYPE (host.HostScene.camera(), blob_camera(blob)).  Keeps the photon maps."""
        cam = np.ascontiguousarray(cam, dtype=CAMERA_DTYPE).reshape(1)
        _check(lib().qa_scene_edit_camera(self._h, cam.ctypes.data))

    def _edit_table(self, fn, first, records, dtype):
        records = np.ascontiguousarray(records, dtype=dtype).reshape(-1)
        _check(fn(self._h, int(first), records.size, records.ctypes.data))
        self._photon_sizes = None   # as an upload: the photon maps are dropped

    def edit_lights(self, first, lights):
        """lights: structured array of LIGHT_DTYPE replacing lights [first, first + len)."""
        self._edit_table(lib().qa_scene_edit_lights, first, lights, LIGHT_DTYPE)

    def edit_materials(self, first, materials):
        """materials: structured array of MATERIAL_DTYPE; texture-map references must stay as they are."""
        self._edit_table(lib().qa_scene_edit_materials, first, materials, MATERIAL_DTYPE)

    def edit_instances(self, first, instances):
        """instances: structured array of INSTANCE_DTYPE; only tm, itm and pos may differ from the resident records."""
        self._edit_table(lib().qa_scene_edit_instances, first, instances, INSTANCE_DTYPE)

    def edit_texmaps(self, first, texmaps):
        """texmaps: structured array of TEXMAP_DTYPE replacing texmaps [first, first + len): itm, pos and the texture a map shows
        (-1 .. number of textures - 1) may change."""
        self._edit_table(lib().qa_scene_edit_texmaps, first, texmaps, TEXMAP_DTYPE)

    def edit_textures(self, first, textures):
        """textures: structured array of TEXTURE_DTYPE; only color1 and color2 may differ from the resident records."""
        self._edit_table(lib().qa_scene_edit_textures, first, textures, TEXTURE_DTYPE)

    def edit_backdrop(self, background=None, environment=None):
        """background / environment: records of TEXCOLOR_DTYPE (blob_backdrop(blob)) or None (stays); the colours may change."""
        recs = [None if r is None else np.ascontiguousarray(r, dtype=TEXCOLOR_DTYPE).reshape(1) for r in (background, environment)]
        _check(lib().qa_scene_edit_backdrop(self._h, *(None if r is None else r.ctypes.data for r in recs)))
        self._photon_sizes = None

    def edit_texels(self, texture, rgb8, origin=(0, 0), stream=None):
        """Replace the texels of file texture `texture` from (x, y) = origin on with rgb8: a numpy (h, w, 3) uint8 array (contiguous
        rows; a row stride is allowed), or a torch uint8 tensor of that shape on the context's device, which is consumed where it
        is (qa_scene_edit_texels_device; stream: the HIP stream handle it was produced on - None: torch's current stream is
        waited for first, as for render_region_device).  Only enqueues."""
        x0, y0 = int(origin[0]), int(origin[1])
        if isinstance(rgb8, np.ndarray):
            rgb8 = _rgb8_rows(rgb8)
            h, w = rgb8.shape[:2]
            _check(lib().qa_scene_edit_texels(self._h, int(texture), x0, y0, x0 + w, y0 + h, rgb8.ctypes.data, rgb8.strides[0]))
        else:
            import torch
            assert rgb8.is_cuda and rgb8.dtype == torch.uint8 and rgb8.dim() == 3 and rgb8.shape[2] == 3 and rgb8.numel() > 0
            if rgb8.stride(2) != 1 or rgb8.stride(1) != 3 or rgb8.stride(0) < 3 * rgb8.shape[1]:
                rgb8 = rgb8.contiguous()
            h, w = rgb8.shape[:2]
            sptr = self._stream_arg(stream, rgb8)
            _check(lib().qa_scene_edit_texels_device(self._h, int(texture), x0, y0, x0 + w, y0 + h, rgb8.data_ptr(), rgb8.stride(0), sptr))
        self._photon_sizes = None

    def download_scene(self):
        """-> the resident scene blob as it now stands (numpy uint8), edits included."""
        n = C.c_uint64()
        lib().qa_scene_download(self._h, None, 0, C.byref(n))
        out = np.zeros(max(int(n.value), 1), np.uint8)
        _check(lib().qa_scene_download(self._h, out.ctypes.data, out.size, C.byref(n)))
        return out[:n.value]

    def scene_stats(self):
        """-> [mesh-table builds, scene device allocations (both since the context was created), bytes copied to the device by
        the last upload or edit, edits since the last upload]."""
        v = (C.c_uint64 * 4)()
        _check(lib().qa_get_scene_stats(self._h, v))
        return [int(x) for x in v]

    # -- photon / caustics maps (the reference's -use-photon-map) ---------------------------------
    def build_photon_maps(self, photon=(10000, 20, 0.2), caustics=(1000, 20, 1.0), seed=DEFAULT_SEED):
        """Trace and balance both maps on the GPU; later renders shade with Scene::usePhotonMap = true.
        photon / caustics: (size, bounce, radius), defaults = RendererParam (src/renderers/renderer.h:51-57)."""
        pp = PhotonParams(PhotonMapParams(*photon), PhotonMapParams(*caustics))
        _check(lib().qa_photon_maps_build(self._h, C.byref(pp), seed))
        self._photon_sizes = (int(photon[0]), int(caustics[0]))

    def clear_photon_maps(self):
        _check(lib().qa_photon_maps_clear(self._h))
        self._photon_sizes = None

    def photon_maps_info(self):
        """-> (emitted[2], emissions[2]): numOfEmittedRays and emission-loop iterations per map."""
        emitted, emissions = (C.c_uint64 * 2)(), (C.c_uint64 * 2)()
        _check(lib().qa_photon_maps_info(self._h, emitted, emissions))
        return list(emitted), list(emissions)

    def download_photon_map(self, which):
        """-> the balanced qa_photon records as they sit in HBM, size + 1 entries ([0] unused)."""
        if self._photon_sizes is None:
            raise HipError(-5, "no photon maps built")
        out = np.zeros(self._photon_sizes[which] + 1, PHOTON_DTYPE)
        _check(lib().qa_photon_maps_download(self._h, which, out.ctypes.data, out.size))
        return out

    # -- rendering -----------------------------------------------------------------------------
    def render_region(self, region, spp, max_bounce=5, seed=DEFAULT_SEED, spp_max=None, stats=False):
        """Synchronous render into host arrays: -> (rgb[h,w,3] f32, depth[h,w] f32, ns[h,w] u32)."""
        x0, y0, x1, y1 = region
        h, w = y1 - y0, x1 - x0
        rgb = np.zeros((h, w, 3), np.float32)
        depth = np.zeros((h, w), np.float32)
        ns = np.zeros((h, w), np.uint32)
        spp_max = spp if spp_max is None else spp_max
        _check(lib().qa_render_region(self._h, x0, y0, x1, y1, spp, spp_max, max_bounce, seed,
                                      QA_RENDER_STATS if stats else 0, rgb.ctypes.data, depth.ctypes.data,
                                      ns.ctypes.data))
        return rgb, depth, ns

    def progressive(self, region, spp, spp_max=None, max_bounce=5, seed=DEFAULT_SEED, stats=False):
        """Begin a progressive frame (qa_progressive_begin): a resident image whose samples are raised in passes
        (Progressive.advance), with a preview between passes.  spp is spp_min; spp_max defaults to it.  The final frame
        is bit-identical to render_region with the same arguments.  One frame per context: a new one ends the last."""
        spp_max = spp if spp_max is None else spp_max
        x0, y0, x1, y1 = region
        _check(lib().qa_progressive_begin(self._h, x0, y0, x1, y1, spp, spp_max, max_bounce, seed,
                                          QA_RENDER_STATS if stats else 0))
        self._prog = Progressive(self, region)
        return self._prog

    def render_region_device(self, region, spp, rgb, depth, ns, max_bounce=5, seed=DEFAULT_SEED, spp_max=None,
                             stats=False, stream=None):
        """Asynchronous render into torch CUDA tensors (float32 [h,w,3], float32 [h,w], int32/uint32 [h,w]).
        stream: a HIP stream handle (e.g. torch.cuda.Stream().cuda_stream).  None or 0 - which is also the
        handle of torch's DEFAULT stream - means the context's own non-blocking stream: call synchronize()
        before anything else consumes the outputs, or pass a real stream and keep the consumers on it."""
        x0, y0, x1, y1 = region
        n = (x1 - x0) * (y1 - y0)
        assert rgb.is_cuda and rgb.is_contiguous() and rgb.numel() == 3 * n and rgb.element_size() == 4
        assert depth.is_cuda and depth.is_contiguous() and depth.numel() == n and depth.element_size() == 4
        assert ns.is_cuda and ns.is_contiguous() and ns.numel() == n and ns.element_size() == 4
        spp_max = spp if spp_max is None else spp_max
        sptr = self._stream_arg(stream, rgb)
        _check(lib().qa_render_region_device(self._h, x0, y0, x1, y1, spp, spp_max, max_bounce, seed,
                                             QA_RENDER_STATS if stats else 0, rgb.data_ptr(), depth.data_ptr(),
                                             ns.data_ptr(), sptr))

    def display_device(self, rgb, depth, ns, spp_max, srgb=True, stream=None, want=DISPLAY_ALL, **given):
        """qa_display_device: the FrameBuffer's 8-bit products of a frame of float results in torch CUDA tensors (float32 [..,3],
        float32, int32/uint32, as render_region_device fills them), computed on the device.  want: the products to make, of
        color / count / zimg / countimg / mask / stats; a tensor passed by that name is written instead of a new one (uint8;
        stats: 16 bytes).  -> dict name -> tensor (None where not wanted); stats_from_tensor() reads the statistics.  Only
        enqueues (see render_region_device for the stream)."""
        n = depth.numel()
        assert rgb.is_cuda and rgb.is_contiguous() and rgb.numel() == 3 * n and rgb.element_size() == 4
        assert depth.is_cuda and depth.is_contiguous() and depth.element_size() == 4
        assert ns.is_cuda and ns.is_contiguous() and ns.numel() == n and ns.element_size() == 4
        out, ptrs = _display_outputs(n, rgb.device, want, given)
        sptr = self._stream_arg(stream, rgb)
        _check(lib().qa_display_device(self._h, rgb.data_ptr(), depth.data_ptr(), ns.data_ptr(), n, int(spp_max), int(bool(srgb)),
                                       *ptrs, sptr))
        return out

    def denoise_device(self, rgb, depth, ns, out=None, params=None, iterations=None, sigma_color=None, sigma_depth=None, stream=None):
        """qa_denoise_device: a filtered copy of a frame of float results in torch CUDA tensors (float32 [h,w,3], float32 [h,w],
        int32/uint32 [h,w]) for display: an edge-avoiding a-trous filter guided by colour and depth (include/qaray_hip.h).  out:
        the float32 [h,w,3] tensor to write (may be rgb itself; None: a new one).  params: a DenoiseParams; the keyword arguments
        override its fields (defaults: the library's).  -> out.  Only enqueues (see render_region_device for the stream).  The
        8-bit picture: display_device(out, depth, ns, spp_max)."""
        (h, w), ptrs, out, _ = _denoise_device_planes(rgb, depth, ns, out)
        p = DenoiseParams.of(params, iterations, sigma_color, sigma_depth)
        _check(lib().qa_denoise_device(self._h, *ptrs[:3], w, h, C.byref(p), out.data_ptr(), self._stream_arg(stream, rgb)))
        return out

    def denoise_guided_device(self, rgb, depth, ns, normal=None, albedo=None, out=None, params=None, iterations=None, sigma_color=None,
                              sigma_depth=None, sigma_normal=None, stream=None):
        """qa_denoise_guided_device: denoise_device guided by the first-hit planes of gbuffer_device as well (float32 [h,w,3] CUDA
        tensors; the flags are the guides given, and with neither the result is denoise_device's).  -> out; only enqueues."""
        (h, w), ptrs, out, flags = _denoise_device_planes(rgb, depth, ns, out, normal, albedo)
        p = DenoiseGuidedParams.of(params, flags, iterations, sigma_color, sigma_depth, sigma_normal)
        _check(lib().qa_denoise_guided_device(self._h, *ptrs[:5], w, h, C.byref(p), out.data_ptr(), self._stream_arg(stream, rgb)))
        return out

    def denoise_variance_device(self, rgb, depth, ns, normal=None, albedo=None, variance=None, out=None, params=None, iterations=None,
                                sigma_color=None, sigma_depth=None, sigma_normal=None, variance_scale=None, stream=None):
        """qa_denoise_variance_device: denoise_guided_device with a per-pixel variance of the luma in place of pass 0's spatial guess
        (include/qaray_hip.h): variance, a float32 [h,w] CUDA tensor, -1 where there is none - TemporalPreview(moments=True).variance
        or the out_variance of reproject_moments_device.  The flags are the planes given; without variance the result is
        denoise_guided_device's.  -> out; only enqueues."""
        (h, w), ptrs, out, flags = _denoise_device_planes(rgb, depth, ns, out, normal, albedo, variance)
        p = DenoiseVarianceParams.of(params, flags, iterations, sigma_color, sigma_depth, sigma_normal, variance_scale)
        _check(lib().qa_denoise_variance_device(self._h, *ptrs, w, h, C.byref(p), out.data_ptr(), self._stream_arg(stream, rgb)))
        return out

    def reproject_device(self, cur, history, prev_cam, cur_cam, origin=(0, 0), ids=None, hist_ids=None, out=None, out_length=None, params=None,
                         depth_tolerance=None, max_history=None, stream=None):
        """qa_reproject_device: the accumulated frame of an earlier camera carried into the frame of the camera as it now stands
        (include/qaray_hip.h), on torch CUDA tensors.  cur = (rgb float32 [h,w,3], depth float32 [h,w], ns int32/uint32 [h,w]) as
        render_region_device fills them under cur_cam; history = (rgb, depth, length float32 [h,w]) accumulated under prev_cam;
        the cameras are records of CAMERA_DTYPE; origin: the image pixel (x0, y0) of the frames' first pixel; ids / hist_ids: the
        int32 [h,w,2] planes of gbuffer_device, both or neither.  out (may be cur's rgb itself) / out_length: the tensors to write
        (None: new ones); neither may be a history plane.  params: a ReprojectParams; the keyword arguments override its fields.
        -> (out, out_length), the history of the next call together with cur's depth and ids.  Only enqueues (see
        render_region_device for the stream)."""
        _, head, keep, out, out_length = _reproject_device_planes(cur, history, prev_cam, cur_cam, origin, ids, hist_ids, out, out_length)
        p = ReprojectParams.of(params, depth_tolerance, max_history)
        sptr = self._stream_arg(stream, out)
        _check(lib().qa_reproject_device(self._h, *head, C.byref(p), _ptr(out), _ptr(out_length), sptr))
        return out, out_length

    def _upload_motion(self, motion, device, stream):
        """_motion_tensor(motion) for a reprojection of this context's -> (its pointer or None, records)."""
        # (kept until the next call: without a stream of the caller's the kernel is not ordered against torch's allocator)
        self._motion_upload, count = _motion_tensor(motion, device, stream)
        return _ptr(self._motion_upload), count

    def reproject_motion_device(self, cur, history, prev_cam, cur_cam, origin=(0, 0), ids=None, hist_ids=None, motion=None, out=None, out_length=None,
                                params=None, depth_tolerance=None, max_history=None, clamp=None, clamp_radius=None, clamp_gamma=None, stream=None):
        """qa_reproject_motion_device: reproject_device that follows moved nodes and clamps stale history (include/qaray_hip.h).
        The arguments of reproject_device, and motion: the table of node_motion() as a numpy array (uploaded on the call's stream)
        or a CUDA tensor of its 64-byte records - given, it sets QA_REPROJECT_MOTION and wants both ids planes; clamp (bool) sets
        or clears QA_REPROJECT_CLAMP (out may then not be cur's rgb), clamp_radius / clamp_gamma override params' values (a
        ReprojectMotionParams).  With neither, the result is reproject_device's.  -> (out, out_length); only enqueues."""
        _, head, keep, out, out_length = _reproject_device_planes(cur, history, prev_cam, cur_cam, origin, ids, hist_ids, out, out_length)
        table, count = self._upload_motion(motion, out.device, stream)
        p = ReprojectMotionParams.of(params, depth_tolerance, max_history, True if motion is not None else None, clamp, clamp_radius, clamp_gamma)
        sptr = self._stream_arg(stream, out)
        _check(lib().qa_reproject_motion_device(self._h, *head, table, count, C.byref(p), _ptr(out), _ptr(out_length), sptr))
        return out, out_length

    def reproject_moments_device(self, cur, history, prev_cam, cur_cam, origin=(0, 0), ids=None, hist_ids=None, hist_moments=None, motion=None, out=None,
                                 out_length=None, out_moments=None, out_variance=None, params=None, depth_tolerance=None, max_history=None, clamp=None,
                                 clamp_radius=None, clamp_gamma=None, moments=None, shorten=None, min_frames=None, shorten_rate=None, stream=None):
        """qa_reproject_moments_device: reproject_motion_device that carries the luma's first two moments and shortens the history
        the clamp moved (include/qaray_hip.h).  The arguments of reproject_motion_device, and hist_moments: float32 [h,w,2], the
        out_moments of the call before (None: nobody has moment history); moments (bool) sets or clears QA_REPROJECT_MOMENTS, which
        writes out_moments [h,w,2] and out_variance [h,w] (None: new ones) - the variance of the accumulated colour's luma, -1 where
        there is none; shorten (bool) sets or clears QA_REPROJECT_SHORTEN (wants clamp); min_frames / shorten_rate override params'
        values (a ReprojectMomentsParams).  With neither flag the result is reproject_motion_device's.
        -> (out, out_length, out_moments, out_variance), the last two None when the flag is clear and they were not given; only
        enqueues."""
        (h, w), head, keep, out, out_length = _reproject_device_planes(cur, history, prev_cam, cur_cam, origin, ids, hist_ids, out, out_length)
        p = ReprojectMomentsParams.of(params, depth_tolerance, max_history, True if motion is not None else None, clamp, clamp_radius, clamp_gamma,
                                      moments, shorten, min_frames, shorten_rate)
        out_moments, out_variance = _moments_tensors(p, h, w, out.device, hist_moments, out_moments, out_variance)
        table, count = self._upload_motion(motion, out.device, stream)
        sptr = self._stream_arg(stream, out)
        _check(lib().qa_reproject_moments_device(self._h, *head, _ptr(hist_moments), table, count, C.byref(p), _ptr(out), _ptr(out_length),
                                                 _ptr(out_moments), _ptr(out_variance), sptr))
        return out, out_length, out_moments, out_variance

    def gbuffer(self, region, seed=DEFAULT_SEED):
        """qa_gbuffer_region: the first-hit guide planes of a region -> dict of numpy arrays: normal [h,w,3] f32 (world space, 0 on a
        miss), albedo [h,w,3] f32, depth [h,w] f32 (render_region's depth plane), ids [h,w,2] i32 (node, material; -1 on a miss;
        QA_GBUFFER_BACKFACE of the material word: a back-face hit).  Synchronises."""
        x0, y0, x1, y1 = region
        h, w = y1 - y0, x1 - x0
        out = {"normal": np.zeros((h, w, 3), np.float32), "albedo": np.zeros((h, w, 3), np.float32), "depth": np.zeros((h, w), np.float32),
               "ids": np.zeros((h, w, 2), np.int32)}
        _check(lib().qa_gbuffer_region(self._h, x0, y0, x1, y1, seed, *(out[k].ctypes.data for k in GBUFFER_PLANES)))
        return out

    def gbuffer_device(self, region, seed=DEFAULT_SEED, normal=None, albedo=None, depth=None, ids=None, stream=None):
        """qa_gbuffer_region_device into torch CUDA tensors (see gbuffer for the shapes): the planes given are written; when none is
        given all four are allocated.  -> dict name -> tensor.  Only enqueues (see render_region_device for the stream)."""
        import torch
        out, ptrs = _output_tensors(GBUFFER_PLANES, *_region_planes(region, GBUFFER_PLANES), torch.device("cuda", self.device_id),
                                    dict(normal=normal, albedo=albedo, depth=depth, ids=ids))
        sptr = self._stream_arg(stream, next(iter(out.values())))
        x0, y0, x1, y1 = region
        _check(lib().qa_gbuffer_region_device(self._h, x0, y0, x1, y1, seed, *ptrs, sptr))
        return out

    def matte(self, region, spp, ns=None):
        """qa_matte_region: the matte planes of a region over the camera rays of all of a pixel's samples -> dict of numpy arrays:
        coverage [h,w] f32 (hits / samples: alpha), albedo [h,w,3] f32 (the running mean of gbuffer's albedo over the samples),
        normal [h,w,3] f32 (the mean hit normal, not normalised; 0 where nothing is hit), backdrop [h,w,3] f32 (the part of a
        frame's colour that came from rays which met nothing).  ns: uint32 [h,w] sample counts (a frame's ns plane): a pixel takes
        min(ns, spp) samples, and 0 gives zeros; None: spp everywhere.  A camera with depth of field is refused.  Synchronises."""
        x0, y0, x1, y1 = region
        h, w = y1 - y0, x1 - x0
        if ns is not None:
            ns = np.ascontiguousarray(ns, dtype=np.uint32)
            if ns.shape != (h, w):
                raise ValueError(f"ns: shape {(h, w)} is expected, not {ns.shape}")
        out = {"coverage": np.zeros((h, w), np.float32), "albedo": np.zeros((h, w, 3), np.float32), "normal": np.zeros((h, w, 3), np.float32),
               "backdrop": np.zeros((h, w, 3), np.float32)}
        _check(lib().qa_matte_region(self._h, x0, y0, x1, y1, int(spp), _ptr(ns), *(out[k].ctypes.data for k in MATTE_PLANES)))
        return out

    def matte_device(self, region, spp, ns=None, coverage=None, albedo=None, normal=None, backdrop=None, stream=None):
        """qa_matte_region_device into torch CUDA tensors (see matte for the shapes; ns: an int32 / uint32 CUDA tensor [h,w] or None):
        the planes given are written; when none is given all four are allocated.  -> dict name -> tensor.  Only enqueues (see
        render_region_device for the stream)."""
        import torch
        out, ptrs = _output_tensors(MATTE_PLANES, *_region_planes(region, MATTE_PLANES), torch.device("cuda", self.device_id),
                                    dict(coverage=coverage, albedo=albedo, normal=normal, backdrop=backdrop))
        x0, y0, x1, y1 = region
        if ns is not None:
            assert ns.is_cuda and ns.is_contiguous() and ns.element_size() == 4 and not ns.dtype.is_floating_point and ns.numel() == (y1 - y0) * (x1 - x0), "ns"
        nptr = None if ns is None else ns.data_ptr()
        sptr = self._stream_arg(stream, next(iter(out.values())))
        _check(lib().qa_matte_region_device(self._h, x0, y0, x1, y1, int(spp), nptr, *ptrs, sptr))
        return out

    def idmatte(self, region, spp, key="node", ns=None):
        """qa_idmatte_region: the id matte of a region over the camera rays of all of a pixel's samples -> dict of numpy arrays: ids
        [h,w,8] i32 and counts [h,w,8] u32 (the nodes - key="node" - or materials - key="material" - the samples meet and how many
        samples each takes, by count descending, then id ascending; free slots QA_IDMATTE_EMPTY, 0), other [h,w] u32 (hits that found
        the table full), samples [h,w] u32.  ns as matte's.  A camera with depth of field is refused.  Synchronises."""
        x0, y0, x1, y1 = region
        h, w = y1 - y0, x1 - x0
        if ns is not None:
            ns = np.ascontiguousarray(ns, dtype=np.uint32)
            if ns.shape != (h, w):
                raise ValueError(f"ns: shape {(h, w)} is expected, not {ns.shape}")
        out = {"ids": np.zeros((h, w, QA_IDMATTE_SLOTS), np.int32), "counts": np.zeros((h, w, QA_IDMATTE_SLOTS), np.uint32),
               "other": np.zeros((h, w), np.uint32), "samples": np.zeros((h, w), np.uint32)}
        _check(lib().qa_idmatte_region(self._h, x0, y0, x1, y1, int(spp), _ptr(ns), _idmatte_key(key), *(out[k].ctypes.data for k in IDMATTE_PLANES)))
        return out

    def idmatte_device(self, region, spp, key="node", ns=None, ids=None, counts=None, other=None, samples=None, stream=None):
        """qa_idmatte_region_device into torch CUDA tensors (see idmatte for the shapes; all four are int32 tensors, the unsigned
        planes' bits; ns: an int32 / uint32 CUDA tensor [h,w] or None): the planes given are written; when none is given all four are
        allocated.  -> dict name -> tensor.  Only enqueues (see render_region_device for the stream)."""
        import torch
        out, ptrs = _output_tensors(IDMATTE_PLANES, *_idmatte_planes(region), torch.device("cuda", self.device_id),
                                    dict(ids=ids, counts=counts, other=other, samples=samples))
        x0, y0, x1, y1 = region
        if ns is not None:
            assert ns.is_cuda and ns.is_contiguous() and ns.element_size() == 4 and not ns.dtype.is_floating_point and ns.numel() == (y1 - y0) * (x1 - x0), "ns"
        nptr = None if ns is None else ns.data_ptr()
        sptr = self._stream_arg(stream, next(iter(out.values())))
        _check(lib().qa_idmatte_region_device(self._h, x0, y0, x1, y1, int(spp), nptr, _idmatte_key(key), *ptrs, sptr))
        return out

    def idmatte_select_device(self, ids, counts, samples, select, out=None, stream=None, out_bytes=None):
        """qa_idmatte_select_device: the coverage plane of the ids of `select` (a sequence of at most QA_IDMATTE_MAX_SELECT ints) from
        the planes idmatte_device wrote: per pixel the counts of the slots whose id is selected, summed, over the pixel's samples; 0
        where it has none.  out: the float32 [h,w] tensor to write (None: a new one) -> out.  out_bytes: a uint8 [h,w] tensor that
        also gets the plane's 8-bit grey picture (the byte display_device makes of the value without sRGB).  Only enqueues (see
        render_region_device for the stream)."""
        import torch
        n = samples.numel()
        for t, k in ((ids, QA_IDMATTE_SLOTS), (counts, QA_IDMATTE_SLOTS), (samples, 1)):
            assert t.is_cuda and t.is_contiguous() and t.element_size() == 4 and not t.dtype.is_floating_point and t.numel() == k * n
        sel = _idmatte_select_list(select)
        if out is None:
            out = torch.empty(tuple(samples.shape), dtype=torch.float32, device=ids.device)
        assert out.is_cuda and out.is_contiguous() and out.dtype == torch.float32 and out.numel() == n
        assert out_bytes is None or (out_bytes.is_cuda and out_bytes.is_contiguous() and out_bytes.dtype == torch.uint8 and out_bytes.numel() == n)
        sptr = self._stream_arg(stream, ids)
        _check(lib().qa_idmatte_select_device(self._h, ids.data_ptr(), counts.data_ptr(), samples.data_ptr(), n, sel.ctypes.data if sel.size else None,
                                              sel.size, out.data_ptr(), _ptr(out_bytes), sptr))
        return out

    def ao(self, region, spp, K=4, radius=float("inf"), first=0, ns=None, seed=DEFAULT_SEED):
        """qa_ao_region: the ambient occlusion of a region (the opening comment of qa_ao_dev.h is the specification): from what the
        camera rays of samples first .. first + spp - 1 of a pixel hit, K cosine-weighted rays over the facing side, each tested as
        occluded() tests a ray of length radius -> dict of numpy arrays open [h,w] u32 (the rays that met nothing), rays [h,w] u32
        (hit samples * K), ao [h,w] f32 (open / rays, 1 where rays is 0).  ns: [h,w] sample counts, a pixel then takes
        min(max(ns - first, 0), spp) samples.  A camera with depth of field is refused.  Synchronises."""
        x0, y0, x1, y1 = region
        h, w = y1 - y0, x1 - x0
        if ns is not None:
            ns = np.ascontiguousarray(ns, dtype=np.uint32)
            if ns.shape != (h, w):
                raise ValueError(f"ns: shape {(h, w)} is expected, not {ns.shape}")
        out = {"open": np.zeros((h, w), np.uint32), "rays": np.zeros((h, w), np.uint32), "ao": np.zeros((h, w), np.float32)}
        _check(lib().qa_ao_region(self._h, x0, y0, x1, y1, int(first), int(spp), _ptr(ns), int(K), float(radius), int(seed) & 0xFFFFFFFF,
                                  *(out[k].ctypes.data for k in AO_PLANES)))
        return out

    def ao_device(self, region, spp, K=4, radius=float("inf"), first=0, ns=None, seed=DEFAULT_SEED, open=None, rays=None, ao=None, stream=None):
        """qa_ao_region_device into torch CUDA tensors (see ao for the planes; open and rays are int32 tensors, the unsigned planes'
        bits; ns: an int32 / uint32 CUDA tensor [h,w] or None): the planes given are written; when none is given all three are
        allocated.  -> dict name -> tensor.  Only enqueues (see render_region_device for the stream)."""
        import torch
        out, ptrs = _output_tensors(AO_PLANES, *_ao_planes(region), torch.device("cuda", self.device_id), dict(open=open, rays=rays, ao=ao))
        x0, y0, x1, y1 = region
        if ns is not None:
            assert ns.is_cuda and ns.is_contiguous() and ns.element_size() == 4 and not ns.dtype.is_floating_point and ns.numel() == (y1 - y0) * (x1 - x0), "ns"
        nptr = None if ns is None else ns.data_ptr()
        sptr = self._stream_arg(stream, next(iter(out.values())))
        _check(lib().qa_ao_region_device(self._h, x0, y0, x1, y1, int(first), int(spp), nptr, int(K), float(radius), int(seed) & 0xFFFFFFFF, *ptrs, sptr))
        return out

    def ao_grey_device(self, ao, out=None, stream=None):
        """qa_ao_grey_device: the 8-bit grey picture of an ao plane (float32 CUDA tensor, any shape): the byte display_device makes of
        the value without sRGB.  out: the uint8 tensor of that shape to write (None: a new one) -> out.  Only enqueues."""
        import torch
        dev = torch.device("cuda", self.device_id)
        _ray_tensor("ao", ao, tuple(ao.shape) if isinstance(ao, torch.Tensor) else (), torch.float32, dev)
        if out is None:
            out = torch.empty(tuple(ao.shape), dtype=torch.uint8, device=dev)
        _ray_tensor("out", out, tuple(ao.shape), torch.uint8, dev)
        _check(lib().qa_ao_grey_device(self._h, ao.data_ptr(), ao.numel(), out.data_ptr(), self._stream_arg(stream, ao)))
        return out

    def ao_points_device(self, points, normals, K=16, radius=float("inf"), first=0, stream_ids=None, seed=DEFAULT_SEED, open=None, ao=None,
                         stream=None):
        """qa_ao_points_device: the ambient occlusion at n points of the caller's (mesh vertices, lightmap texels).  points, normals:
        float32 [n,3] contiguous CUDA tensors, world space, the normals of unit length; point i casts the K rays of the counters
        first .. first + K - 1 of stream i, or stream_ids[i] (int32 [n]).  Outputs: open int32 [n] (the unsigned count's bits), ao
        float32 [n] = open / K; the ones given are written, and when none is given both are allocated.  A point with a component that
        is not finite, or a zero normal, answers open = K, ao = 1.  -> dict name -> tensor.  Only enqueues."""
        import torch
        dev = torch.device("cuda", self.device_id)
        n = _ray_count("points", points) if isinstance(points, torch.Tensor) else 0
        _ray_tensor("points", points, (n, 3), torch.float32, dev)
        _ray_tensor("normals", normals, (n, 3), torch.float32, dev)
        if stream_ids is not None:
            _ray_tensor("stream_ids", stream_ids, (n,), torch.int32, dev)
        out, ptrs = _output_tensors(("open", "ao"), {"open": (n,), "ao": (n,)}, {"open": torch.int32, "ao": torch.float32}, dev, dict(open=open, ao=ao))
        sptr = self._stream_arg(stream, points)
        _check(lib().qa_ao_points_device(self._h, n, points.data_ptr(), normals.data_ptr(), None if stream_ids is None else stream_ids.data_ptr(),
                                         int(first), int(K), float(radius), int(seed) & 0xFFFFFFFF, *ptrs, sptr))
        return out

    def ao_points(self, points, normals, K=16, radius=float("inf"), first=0, stream_ids=None, seed=DEFAULT_SEED):
        """qa_ao_points: ao_points_device from and to host memory.  points, normals: [n,3], converted to float32; stream_ids: [n]
        integers below 2^32 or None -> dict of numpy arrays open [n] u32, ao [n] f32.  Synchronises."""
        p, nr, n = _ray_arrays(points, normals)
        sid = None
        if stream_ids is not None:
            sid = np.ascontiguousarray(np.asarray(stream_ids).astype(np.uint32)).view(np.int32).reshape(-1)
            if sid.shape != (n,):
                raise ValueError(f"stream_ids: shape ({n},) is expected, not {sid.shape}")
        out = {"open": np.zeros(n, np.uint32), "ao": np.zeros(n, np.float32)}
        _check(lib().qa_ao_points(self._h, n, p.ctypes.data, nr.ctypes.data, _ptr(sid), int(first), int(K), float(radius), int(seed) & 0xFFFFFFFF,
                                  out["open"].ctypes.data, out["ao"].ctypes.data))
        return out

    # -- bake maps (qa_bake.hip) --------------------------------------------------------------------
    def bake_texels_device(self, node, width, height, texmap=None, mtl=-1, point=None, normal=None, face=None, bary=None, stream=None):
        """qa_bake_texels_device: the surface point of node `node` (a mesh with texture vertices, or a plane) behind every texel of a
        width x height texture laid over it (the opening comment of qa_bake_dev.h is the specification).  texmap: the scene's texmap
        whose transform the texture vertices go through (None: the raw uv); mtl: only the faces of that material index (-1: all).
        Outputs, contiguous CUDA tensors, row 0 the top row as stored: point, normal float32 [h,w,3] (world space), face int32 [h,w]
        (the blob's face id, -1 where nothing covers the texel: the other planes then hold zeros), bary float32 [h,w,2]; the ones
        given are written, and when none is given all four are allocated.  -> dict name -> tensor.  Only enqueues (see
        render_region_device for the stream)."""
        import torch
        dev = torch.device("cuda", self.device_id)
        w, h = _bake_size(width, height)
        shapes = {"point": (h, w, 3), "normal": (h, w, 3), "face": (h, w), "bary": (h, w, 2)}
        dtypes = {k: torch.int32 if k == "face" else torch.float32 for k in BAKE_PLANES}
        out, ptrs = _output_tensors(BAKE_PLANES, shapes, dtypes, dev, dict(point=point, normal=normal, face=face, bary=bary))
        sptr = self._stream_arg(stream, next(iter(out.values())))
        _check(lib().qa_bake_texels_device(self._h, int(node), -1 if texmap is None else int(texmap), int(mtl), w, h, *ptrs, sptr))
        return out

    def bake_texels(self, node, width, height, texmap=None, mtl=-1, planes=None):
        """qa_bake_texels: bake_texels_device to host memory -> dict of numpy arrays point [h,w,3] f32, normal [h,w,3] f32, face
        [h,w] i32, bary [h,w,2] f32 (planes: the names wanted; None: all four).  Synchronises."""
        w, h = _bake_size(width, height)
        out = _bake_host_planes(w, h, planes)
        _check(lib().qa_bake_texels(self._h, int(node), -1 if texmap is None else int(texmap), int(mtl), w, h,
                                    *(out[k].ctypes.data if k in out else None for k in BAKE_PLANES)))
        return out

    def bake_dilate_device(self, rgb8, face, radius=2, out=None, stream=None):
        """qa_bake_dilate_device: the gutter fill of a baked picture.  rgb8 uint8 [h,w,3], face int32 [h,w] (bake_texels_device's
        plane), contiguous CUDA tensors: a texel with face >= 0 keeps its bytes, another takes those of the nearest covered texel
        within `radius` (<= 8) texels per axis, wrapping at the borders as the texture lookup wraps (ties: dy ascending, then dx);
        with none in reach it keeps its own.  out: the uint8 [h,w,3] tensor to write, not rgb8 (None: a new one) -> out.  Only
        enqueues."""
        import torch
        dev = torch.device("cuda", self.device_id)
        shape = tuple(rgb8.shape) if isinstance(rgb8, torch.Tensor) else ()
        if len(shape) != 3 or shape[2] != 3:
            raise ValueError(f"rgb8: shape (h, w, 3) is expected, not {shape}")
        _ray_tensor("rgb8", rgb8, shape, torch.uint8, dev)
        _ray_tensor("face", face, shape[:2], torch.int32, dev)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=dev)
        _ray_tensor("out", out, shape, torch.uint8, dev)
        _check(lib().qa_bake_dilate_device(self._h, rgb8.data_ptr(), face.data_ptr(), shape[1], shape[0], int(radius), out.data_ptr(),
                                           self._stream_arg(stream, rgb8)))
        return out

    def bake_ao(self, node, texmap, K=64, radius=float("inf"), mtl=-1, dilate=2, seed=DEFAULT_SEED, stream=None):
        """The ambient occlusion of node `node` baked into the file texture of texmap `texmap`, in place: the map of the texture's
        texels (bake_texels_device at the texture's size, through the texmap), ao_points_device at the covered texels' points and
        normals with stream_ids = iy * W + ix, ao_grey_device, the grey in all three channels; uncovered texels keep the texture's
        bytes as they stand, then take their nearest covered neighbour's within `dilate` texels (bake_dilate_device; 0: no fill);
        the picture then replaces the texture's texels (edit_texels).  A composition of those calls, all on one stream: the planes
        stay on the device, only the texture's present bytes are read through download_scene.  -> dict of CUDA tensors ao [H,W]
        f32 (1 where uncovered), face [H,W] i32, rgb8 [H,W,3] u8 (what the texture now holds).  QA_EINVAL for a texmap without a
        file texture.  download_scene comes first (it synchronises where a texture was last edited from device memory, as after an
        earlier bake_ao); the device work is then only enqueued, on `stream` (a HIP stream handle) or, with None, on a side stream
        that torch's current stream is made to wait for."""
        import torch
        dev = torch.device("cuda", self.device_id)
        blob = self.download_scene()
        maps = blob_table(blob, "texmaps")
        if texmap is None or not 0 <= int(texmap) < len(maps) or int(maps[int(texmap)]["texture"]) < 0:
            raise HipError(-1, "bake_ao: the texmap is out of range or has no texture")
        tex = int(maps[int(texmap)]["texture"])
        rec = blob_table(blob, "textures")[tex]
        if int(rec["type"]) != QA_TEX_FILE:
            raise HipError(-1, "bake_ao: the texmap's texture is not a file texture")
        W, H = int(rec["width"]), int(rec["height"])
        # one stream for the library's calls and torch's own steps between them.  stream = None: a side stream of torch's (the
        # context's own stream is not torch's to enqueue on) that starts behind torch's current stream, which in turn waits for it
        cur = torch.cuda.current_stream(dev)
        if stream:
            ts = torch.cuda.ExternalStream(int(stream), device=dev)
        else:
            if self._bake_stream is None:
                self._bake_stream = torch.cuda.Stream(dev)
            ts = self._bake_stream
            ts.wait_stream(cur)
        sptr = ts.cuda_stream
        with torch.cuda.stream(ts):
            current = torch.from_numpy(blob_texels(blob, tex).copy()).to(dev)
            m = self.bake_texels_device(node, W, H, texmap=texmap, mtl=mtl, point=torch.empty((H, W, 3), dtype=torch.float32, device=dev),
                                        normal=torch.empty((H, W, 3), dtype=torch.float32, device=dev),
                                        face=torch.empty((H, W), dtype=torch.int32, device=dev), stream=sptr)
            ids = torch.arange(H * W, dtype=torch.int32, device=dev)
            ao = self.ao_points_device(m["point"].reshape(-1, 3), m["normal"].reshape(-1, 3), K, radius, 0, ids, seed,
                                       ao=torch.empty(H * W, dtype=torch.float32, device=dev), stream=sptr)["ao"].reshape(H, W)
            covered = m["face"] >= 0   # (an uncovered texel's normal is zero: a void point, whose ao is 1)
            grey = self.ao_grey_device(ao, stream=sptr)
            rgb8 = torch.where(covered.unsqueeze(2), grey.unsqueeze(2).expand(H, W, 3), current).contiguous()
            if int(dilate) > 0:
                rgb8 = self.bake_dilate_device(rgb8, m["face"], int(dilate), stream=sptr)
            self.edit_texels(tex, rgb8, stream=sptr)
        out = {"ao": ao, "face": m["face"], "rgb8": rgb8}
        if not stream:
            cur.wait_stream(ts)
            for t in out.values():
                t.record_stream(cur)
        return out

    def bake_light(self, node, texmap, spp=64, max_bounce=5, scale=1.0, mtl=-1, dilate=2, seed=DEFAULT_SEED, stream=None, **options):
        """The light arriving at node `node` baked into the file texture of texmap `texmap`, in place - a light map, composed as
        bake_ao composes its map: the map of the texture's texels (bake_texels_device at the texture's size, through the texmap),
        irradiance_points_device at the texels' points and normals with stream_ids = iy * W + ix (an uncovered texel's normal is
        zero: a void point, black), ao_grey_device of light * scale - linear bytes, which the texel table decodes by / 255
        (texels_host) - uncovered texels keep the texture's bytes as they stand, then take their nearest covered neighbour's within
        `dilate` texels (bake_dilate_device; 0: no fill); the picture then replaces the texture's texels (edit_texels).  The baked
        value is what a frame shows for a white diffuse surface there (kd * light for another colour): not scaled by pi, every
        light weighted 1 / num_lights; values above 1 / scale clip.  The limit: paths that return to the node read its texture as
        it stands during the bake, not the light map being made.  All on one stream, as bake_ao.  -> dict of CUDA tensors light
        [H,W,3] f32 (0 where uncovered), face [H,W] i32, rgb8 [H,W,3] u8 (what the texture now holds).  QA_EINVAL for a texmap
        without a file texture.  One more keyword, photon_maps=False: the same composition with the flag on its point query
        (irradiance_points_device), so that the light map holds the caustics a frame with maps shows; the maps must be built.  The
        last step, edit_texels, drops the maps as every texel edit does: the caller rebuilds them afterwards
        (build_photon_maps), and photon_maps_info() raises until then."""
        import torch
        photon_maps = _photon_maps_option("bake_light", options)
        dev = torch.device("cuda", self.device_id)
        blob = self.download_scene()
        maps = blob_table(blob, "texmaps")
        if texmap is None or not 0 <= int(texmap) < len(maps) or int(maps[int(texmap)]["texture"]) < 0:
            raise HipError(-1, "bake_light: the texmap is out of range or has no texture")
        tex = int(maps[int(texmap)]["texture"])
        rec = blob_table(blob, "textures")[tex]
        if int(rec["type"]) != QA_TEX_FILE:
            raise HipError(-1, "bake_light: the texmap's texture is not a file texture")
        W, H = int(rec["width"]), int(rec["height"])
        cur = torch.cuda.current_stream(dev)   # (the streams: see bake_ao)
        if stream:
            ts = torch.cuda.ExternalStream(int(stream), device=dev)
        else:
            if self._bake_stream is None:
                self._bake_stream = torch.cuda.Stream(dev)
            ts = self._bake_stream
            ts.wait_stream(cur)
        sptr = ts.cuda_stream
        with torch.cuda.stream(ts):
            current = torch.from_numpy(blob_texels(blob, tex).copy()).to(dev)
            m = self.bake_texels_device(node, W, H, texmap=texmap, mtl=mtl, point=torch.empty((H, W, 3), dtype=torch.float32, device=dev),
                                        normal=torch.empty((H, W, 3), dtype=torch.float32, device=dev),
                                        face=torch.empty((H, W), dtype=torch.int32, device=dev), stream=sptr)
            ids = torch.arange(H * W, dtype=torch.int32, device=dev)
            light = self.irradiance_points_device(m["point"].reshape(-1, 3), m["normal"].reshape(-1, 3), spp, max_bounce, seed, ids,
                                                  stream=sptr, photon_maps=photon_maps)[0].reshape(H, W, 3)
            covered = m["face"] >= 0
            grey = self.ao_grey_device(light * float(scale), stream=sptr)
            rgb8 = torch.where(covered.unsqueeze(2), grey, current).contiguous()
            if int(dilate) > 0:
                rgb8 = self.bake_dilate_device(rgb8, m["face"], int(dilate), stream=sptr)
            self.edit_texels(tex, rgb8, stream=sptr)
        out = {"light": light, "face": m["face"], "rgb8": rgb8}
        if not stream:
            cur.wait_stream(ts)
            for t in out.values():
                t.record_stream(cur)
        return out

    def rgba_device(self, rgb, backdrop, coverage, ns, srgb=True, out=None, stream=None):
        """qa_matte_rgba_device: the straight-alpha 8-bit RGBA picture of a frame (rgb float32 [h,w,3] and ns int32 / uint32 [h,w] as
        render_region_device fills them, backdrop and coverage as matte_device(region, spp, ns=ns) does), what a PNG stores: the
        colour is (rgb - backdrop) / coverage, alpha the coverage, pixels with ns == 0 are 0, 0, 0, 0.  out: the uint8 [h,w,4]
        tensor to write (None: a new one) -> out.  Only enqueues (see render_region_device for the stream)."""
        import torch
        n = coverage.numel()
        for t, k in ((rgb, 3), (backdrop, 3), (coverage, 1)):
            assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 and t.numel() == k * n
        assert ns.is_cuda and ns.is_contiguous() and ns.numel() == n and ns.element_size() == 4 and not ns.dtype.is_floating_point
        if out is None:
            out = torch.empty(tuple(coverage.shape) + (4,), dtype=torch.uint8, device=rgb.device)
        assert out.is_cuda and out.is_contiguous() and out.dtype == torch.uint8 and out.numel() == 4 * n
        sptr = self._stream_arg(stream, rgb)
        _check(lib().qa_matte_rgba_device(self._h, rgb.data_ptr(), backdrop.data_ptr(), coverage.data_ptr(), ns.data_ptr(), n, int(bool(srgb)),
                                          out.data_ptr(), sptr))
        return out

    # -- ray queries (qa_ray_query.hip) -----------------------------------------------------------
    def cast_rays_device(self, origins, dirs, t=None, ids=None, normal=None, point=None, stream=None):
        """qa_cast_rays_device: the closest hit of n rays of the caller's, as a path segment of the renderer with that ray meets it.
        origins, dirs: float32 [n,3] contiguous CUDA tensors, world space; dirs are not normalised and t is the parameter along
        them.  Outputs: t float32 [n] (QA_RAY_MISS on a miss), ids int32 [n,2] (node, material word as gbuffer's ids), normal and
        point float32 [n,3] (0 on a miss); the ones given are written, and when none is given all four are allocated.
        -> dict name -> tensor.  Only enqueues (see render_region_device for the stream)."""
        import torch
        dev = torch.device("cuda", self.device_id)
        n = _ray_count("origins", origins) if isinstance(origins, torch.Tensor) else 0
        _ray_tensor("origins", origins, (n, 3), torch.float32, dev)
        _ray_tensor("dirs", dirs, (n, 3), torch.float32, dev)
        shapes = {"t": (n,), "ids": (n, 2), "normal": (n, 3), "point": (n, 3)}
        dtypes = {k: torch.int32 if k == "ids" else torch.float32 for k in RAY_OUTPUTS}
        out, ptrs = _output_tensors(RAY_OUTPUTS, shapes, dtypes, dev, dict(t=t, ids=ids, normal=normal, point=point))
        sptr = self._stream_arg(stream, origins)
        _check(lib().qa_cast_rays_device(self._h, n, origins.data_ptr(), dirs.data_ptr(), *ptrs, sptr))
        return out

    def cast_rays(self, origins, dirs):
        """qa_cast_rays: cast_rays_device from and to host memory.  origins, dirs: [n,3], converted to float32
        -> dict of numpy arrays t [n] f32, ids [n,2] i32, normal [n,3] f32, point [n,3] f32.  Synchronises."""
        o, d, n = _ray_arrays(origins, dirs)
        out = {"t": np.zeros(n, np.float32), "ids": np.zeros((n, 2), np.int32), "normal": np.zeros((n, 3), np.float32),
               "point": np.zeros((n, 3), np.float32)}
        _check(lib().qa_cast_rays(self._h, n, o.ctypes.data, d.ctypes.data, *(out[k].ctypes.data for k in RAY_OUTPUTS)))
        return out

    def occluded_device(self, origins, dirs, tmax, out=None, stream=None):
        """qa_occluded_device: out[i] = 1 where ray i meets a surface before the parameter tmax[i] (what a shadow ray of that length
        answers), else 0.  origins, dirs as cast_rays_device; tmax: a float32 [n] CUDA tensor, or a number for every ray; out: a
        uint8 [n] CUDA tensor, allocated when not given -> out.  Only enqueues.  A number is broadcast into a float32 [n] tensor
        that the context keeps (4 n bytes of device memory) until the next call with a number, or until close(): without a stream
        of the caller's the kernel is not ordered against torch's allocator, which must not hand the memory out before it ran."""
        import torch
        dev = torch.device("cuda", self.device_id)
        n = _ray_count("origins", origins) if isinstance(origins, torch.Tensor) else 0
        _ray_tensor("origins", origins, (n, 3), torch.float32, dev)
        _ray_tensor("dirs", dirs, (n, 3), torch.float32, dev)
        if out is None:
            out = torch.empty(n, dtype=torch.uint8, device=dev)
        _ray_tensor("out", out, (n,), torch.uint8, dev)
        if isinstance(tmax, (int, float, np.floating, np.integer)):
            ts = torch.cuda.ExternalStream(stream, device=dev) if stream else torch.cuda.current_stream(dev)
            with torch.cuda.stream(ts):
                tmax = torch.full((n,), float(tmax), dtype=torch.float32, device=dev)
            self._tmax_fill = tmax
        _ray_tensor("tmax", tmax, (n,), torch.float32, dev)
        sptr = self._stream_arg(stream, origins)
        _check(lib().qa_occluded_device(self._h, n, origins.data_ptr(), dirs.data_ptr(), tmax.data_ptr(), out.data_ptr(), sptr))
        return out

    def occluded(self, origins, dirs, tmax):
        """qa_occluded: occluded_device from and to host memory; tmax: [n], or a number for every ray -> uint8 [n].  Synchronises."""
        o, d, n = _ray_arrays(origins, dirs)
        tm = np.asarray(tmax, dtype=np.float32)
        if tm.ndim == 0:
            tm = np.full(n, tm, np.float32)
        if tm.shape != (n,):
            raise ValueError(f"tmax: a number or shape ({n},) is expected, not {tm.shape}")
        tm = np.ascontiguousarray(tm)
        out = np.zeros(n, np.uint8)
        _check(lib().qa_occluded(self._h, n, o.ctypes.data, d.ctypes.data, tm.ctypes.data, out.ctypes.data))
        return out

    def camera_rays_device(self, region, seed=DEFAULT_SEED, origins=None, dirs=None, stream=None):
        """qa_camera_rays_device: the camera rays of sample 0 of the pixels of a region, exactly as a frame of that seed builds them
        -> (origins, dirs): float32 [h*w,3] CUDA tensors, region-local and row-major (given, or allocated); dirs are unit vectors.
        cast_rays_device of them meets what the frame's first sample meets.  Only enqueues."""
        import torch
        dev = torch.device("cuda", self.device_id)
        x0, y0, x1, y1 = (int(v) for v in region)
        n = max(x1 - x0, 0) * max(y1 - y0, 0)   # (an empty region is the library's to refuse)
        origins = torch.empty((n, 3), dtype=torch.float32, device=dev) if origins is None else origins
        dirs = torch.empty((n, 3), dtype=torch.float32, device=dev) if dirs is None else dirs
        _ray_tensor("origins", origins, (n, 3), torch.float32, dev)
        _ray_tensor("dirs", dirs, (n, 3), torch.float32, dev)
        sptr = self._stream_arg(stream, origins)
        _check(lib().qa_camera_rays_device(self._h, x0, y0, x1, y1, seed, origins.data_ptr() or None, dirs.data_ptr() or None, sptr))
        return origins, dirs

    def camera_rays(self, region, seed=DEFAULT_SEED):
        """camera_rays_device to host memory -> (origins, dirs): numpy float32 [h*w,3].  Synchronises."""
        o, d = self.camera_rays_device(region, seed)
        self.synchronize()
        return o.cpu().numpy(), d.cpu().numpy()

    # -- radiance queries (qa_radiance.hip) --------------------------------------------------------
    def radiance_rays_device(self, origins, dirs, spp=1, max_bounce=5, seed=DEFAULT_SEED, dx=None, dy=None, screen=None, stream_ids=None,
                             miss_environment=False, rgb=None, t=None, ns=None, stream=None, photon_maps=False):
        """qa_radiance_rays_device: n rays of the caller's path-traced by the renderer's integrator, spp samples each.  origins, dirs:
        float32 contiguous CUDA tensors, [n,3] (every sample of ray q starts from ray q) or [n,spp,3] (rays per sample:
        QA_RADIANCE_PER_SAMPLE); dirs are used as given (unit length is assumed).  Optional, shaped as origins: dx, dy the
        differential directions (both or neither; without them textures at the first hit are looked up unfiltered), screen
        [...,2] where a missed first ray looks a background image up (pixels).  stream_ids: int32 or uint32 [n], the random-number
        stream of each ray (None: the ray's index).  miss_environment: a missed first ray takes the environment by direction
        and not the background.  Outputs (given, or allocated): rgb float32 [n,3], t float32 [n] (QA_RAY_MISS on a miss), ns
        int32 [n] (spp for a finished ray) -> (rgb, t, ns).  photon_maps (QA_RADIANCE_PHOTON_MAPS): the paths gather from the
        photon and caustics maps build_photon_maps made, exactly as a frame does while they are built; opt-in - without it a
        context with maps refuses the call (QA_EUNSUPPORTED), with it one without maps does (QA_ENOSCENE).  Only enqueues (see
        render_region_device for the stream)."""
        import torch
        dev = torch.device("cuda", self.device_id)
        if not isinstance(origins, torch.Tensor):
            raise TypeError(f"origins: a torch tensor is expected, not {type(origins).__name__}")
        spp = int(spp)
        n, per_sample = _radiance_shape("origins", origins, spp)
        rec = (n, spp) if per_sample else (n,)
        _ray_tensor("origins", origins, rec + (3,), torch.float32, dev)
        _ray_tensor("dirs", dirs, rec + (3,), torch.float32, dev)
        if (dx is None) != (dy is None):
            raise ValueError("dx and dy: both or neither")
        for name, a, last in (("dx", dx, 3), ("dy", dy, 3), ("screen", screen, 2)):
            if a is not None:
                _ray_tensor(name, a, rec + (last,), torch.float32, dev)
        if stream_ids is not None:
            if isinstance(stream_ids, torch.Tensor) and stream_ids.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)):
                raise TypeError(f"stream_ids: dtype torch.int32 or torch.uint32 is expected, not {stream_ids.dtype}")
            _ray_tensor("stream_ids", stream_ids, (n,), getattr(stream_ids, "dtype", None), dev)
        rgb = torch.empty((n, 3), dtype=torch.float32, device=dev) if rgb is None else rgb
        t = torch.empty((n,), dtype=torch.float32, device=dev) if t is None else t
        ns = torch.empty((n,), dtype=torch.int32, device=dev) if ns is None else ns
        _ray_tensor("rgb", rgb, (n, 3), torch.float32, dev)
        _ray_tensor("t", t, (n,), torch.float32, dev)
        _ray_tensor("ns", ns, (n,), torch.int32, dev)
        p = RadianceParams.of(spp, max_bounce, seed, per_sample, miss_environment, photon_maps)
        sptr = self._stream_arg(stream, origins)
        ptr = lambda a: None if a is None else (a.data_ptr() or None)   # noqa: E731
        _check(lib().qa_radiance_rays_device(self._h, n, ptr(origins), ptr(dirs), ptr(dx), ptr(dy), ptr(screen), ptr(stream_ids), C.byref(p),
                                             ptr(rgb), ptr(t), ptr(ns), sptr))
        return rgb, t, ns

    def radiance_rays(self, origins, dirs, spp=1, max_bounce=5, seed=DEFAULT_SEED, dx=None, dy=None, screen=None, stream_ids=None,
                      miss_environment=False, photon_maps=False):
        """qa_radiance_rays: radiance_rays_device from and to host memory.  Arrays as there, converted to float32 (stream_ids to
        uint32); photon_maps as there -> (rgb [n,3] f32, t [n] f32, ns [n] u32) numpy arrays.  Synchronises."""
        spp = int(spp)
        o = np.ascontiguousarray(origins, dtype=np.float32)
        n, per_sample = _radiance_shape("origins", o, spp)
        rec = (n, spp) if per_sample else (n,)
        if (dx is None) != (dy is None):
            raise ValueError("dx and dy: both or neither")
        arrs = {}
        for name, a, last in (("dirs", dirs, 3), ("dx", dx, 3), ("dy", dy, 3), ("screen", screen, 2)):
            if a is None:
                arrs[name] = None
                continue
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.shape != rec + (last,):
                raise ValueError(f"{name}: shape {rec + (last,)} is expected, not {a.shape}")
            arrs[name] = a
        if arrs["dirs"] is None:
            raise TypeError("dirs: an array is expected")
        sid = None
        if stream_ids is not None:
            sid = np.ascontiguousarray(stream_ids, dtype=np.uint32)
            if sid.shape != (n,):
                raise ValueError(f"stream_ids: shape ({n},) is expected, not {sid.shape}")
        rgb, t, ns = np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros(n, np.uint32)
        p = RadianceParams.of(spp, max_bounce, seed, per_sample, miss_environment, photon_maps)
        ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
        _check(lib().qa_radiance_rays(self._h, n, ptr(o), ptr(arrs["dirs"]), ptr(arrs["dx"]), ptr(arrs["dy"]), ptr(arrs["screen"]), ptr(sid),
                                      C.byref(p), ptr(rgb), ptr(t), ptr(ns)))
        return rgb, t, ns

    # -- irradiance queries (qa_irradiance.hip) ----------------------------------------------------
    def irradiance_points_device(self, points, normals, spp=16, max_bounce=5, seed=DEFAULT_SEED, stream_ids=None, rgb=None, ns=None, stream=None,
                                 **options):
        """qa_irradiance_points_device: the light arriving at n surface points of the caller's (lightmap texels, mesh vertices),
        path-traced by the renderer's integrator started at the points, spp samples each: the direct light at the point, one
        cosine-weighted bounce, and the integrator as it stands behind it.  kd * rgb is what a frame shows for a diffuse surface
        of colour kd there (not scaled by pi; every light weighs 1 / num_lights).  points, normals: float32 [n,3] contiguous CUDA
        tensors, world space, the normals of unit length (used as given).  stream_ids: int32 or uint32 [n], the random-number
        stream of each point (None: the point's index).  A point with a component that is not finite, or a zero normal, is black.
        Outputs (given, or allocated): rgb float32 [n,3], ns int32 [n] (spp for a finished point) -> (rgb, ns).  One more
        keyword, photon_maps=False (QA_RADIANCE_PHOTON_MAPS): the point gathers from the caustics map ahead of its direct light,
        and the paths behind its bounce gather from both maps as a frame's do while build_photon_maps' maps are built; opt-in -
        without it a context with maps refuses the call (QA_EUNSUPPORTED), with it one without maps does (QA_ENOSCENE).  Only
        enqueues (see render_region_device for the stream)."""
        import torch
        photon_maps = _photon_maps_option("irradiance_points_device", options)
        dev = torch.device("cuda", self.device_id)
        if not isinstance(points, torch.Tensor):
            raise TypeError(f"points: a torch tensor is expected, not {type(points).__name__}")
        n = _ray_count("points", points)
        _ray_tensor("points", points, (n, 3), torch.float32, dev)
        _ray_tensor("normals", normals, (n, 3), torch.float32, dev)
        if stream_ids is not None:
            if isinstance(stream_ids, torch.Tensor) and stream_ids.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)):
                raise TypeError(f"stream_ids: dtype torch.int32 or torch.uint32 is expected, not {stream_ids.dtype}")
            _ray_tensor("stream_ids", stream_ids, (n,), getattr(stream_ids, "dtype", None), dev)
        rgb = torch.empty((n, 3), dtype=torch.float32, device=dev) if rgb is None else rgb
        ns = torch.empty((n,), dtype=torch.int32, device=dev) if ns is None else ns
        _ray_tensor("rgb", rgb, (n, 3), torch.float32, dev)
        _ray_tensor("ns", ns, (n,), torch.int32, dev)
        p = RadianceParams.of(spp, max_bounce, seed, photon_maps=photon_maps)
        sptr = self._stream_arg(stream, points)
        ptr = lambda a: None if a is None else (a.data_ptr() or None)   # noqa: E731
        _check(lib().qa_irradiance_points_device(self._h, n, ptr(points), ptr(normals), ptr(stream_ids), C.byref(p), ptr(rgb), ptr(ns), sptr))
        return rgb, ns

    def irradiance_points(self, points, normals, spp=16, max_bounce=5, seed=DEFAULT_SEED, stream_ids=None, **options):
        """qa_irradiance_points: irradiance_points_device from and to host memory.  points, normals: [n,3], converted to float32;
        stream_ids: [n] integers below 2^32 or None; the keyword photon_maps=False as there -> (rgb [n,3] f32, ns [n] u32) numpy
        arrays.  Synchronises."""
        photon_maps = _photon_maps_option("irradiance_points", options)
        p, nr, n = _ray_arrays(points, normals)
        sid = None
        if stream_ids is not None:
            sid = np.ascontiguousarray(stream_ids, dtype=np.uint32)
            if sid.shape != (n,):
                raise ValueError(f"stream_ids: shape ({n},) is expected, not {sid.shape}")
        rgb, ns = np.zeros((n, 3), np.float32), np.zeros(n, np.uint32)
        par = RadianceParams.of(spp, max_bounce, seed, photon_maps=photon_maps)
        _check(lib().qa_irradiance_points(self._h, n, p.ctypes.data, nr.ctypes.data, _ptr(sid), C.byref(par), rgb.ctypes.data, ns.ctypes.data))
        return rgb, ns

    # -- light probes (qa_lightprobe.hip) ----------------------------------------------------------
    def probe_sh_device(self, points, m=16, spp=1, max_bounce=5, seed=DEFAULT_SEED, jitter=False, photon_maps=False, stream_ids=None, sh=None,
                        cube=None, hits=None, tmin=None, chunk_rays=0, stream=None):
        """qa_probe_sh_device: the light arriving at n points in free space, as order-2 spherical harmonics.  A probe is a cube map
        of m x m texels per face around its point: K = 6 m^2 rays through the texel centres (jitter: jittered inside the texels),
        each path-traced by the renderer's integrator as radiance_rays_device traces a ray (miss_environment, spp samples, the
        stream (S * K + k) mod 2^32 for the probe's stream id S), weighted by its texel's solid angle and projected on the device.
        It holds what a camera at the point would see in every direction - emitters, the environment, the surfaces around it under
        their own direct and bounced light - and not the direct term of point, spot and directional lights at the point itself: a
        shader adds those analytically.  points: float32 [n,3] contiguous CUDA tensor; stream_ids: int32 or uint32 [n] (None: the
        probe's index).  Outputs (given, or allocated; cube only when given or cube=True): sh float32 [n,9,3], cube float32
        [n,6,m,m,3] the rays' rgb, hits int32 [n] the rays that hit something, tmin float32 [n] the nearest hit (QA_RAY_MISS for
        none) -> dict of them.  A point that is not finite gives zeros.  photon_maps as radiance_rays_device's; chunk_rays: the
        rays traced at a time (0: 2^20), which bounds the scratch and changes no result.  Only enqueues (see render_region_device
        for the stream)."""
        return self._probe_sh_device(points, m, spp, max_bounce, seed, jitter, photon_maps, stream_ids, sh, cube, hits, tmin, chunk_rays, stream)

    def _probe_sh_device(self, points, m, spp, max_bounce, seed, jitter, photon_maps, stream_ids, sh, cube, hits, tmin, chunk_rays, stream, vis=None,
                         moments=None):
        """probe_sh_device, and with vis (ProbeVisParams) probevis_sh_device: the same arguments, checks and outputs, and the moments"""
        import torch
        dev = torch.device("cuda", self.device_id)
        if not isinstance(points, torch.Tensor):
            raise TypeError(f"points: a torch tensor is expected, not {type(points).__name__}")
        n = _ray_count("points", points)
        _ray_tensor("points", points, (n, 3), torch.float32, dev)
        m = int(m)
        if not 1 <= m <= QA_PROBE_MAX_M:
            raise ValueError(f"m: 1 .. {QA_PROBE_MAX_M} is expected, not {m}")
        if stream_ids is not None:
            if isinstance(stream_ids, torch.Tensor) and stream_ids.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)):
                raise TypeError(f"stream_ids: dtype torch.int32 or torch.uint32 is expected, not {stream_ids.dtype}")
            _ray_tensor("stream_ids", stream_ids, (n,), getattr(stream_ids, "dtype", None), dev)
        sh = torch.empty((n, 9, 3), dtype=torch.float32, device=dev) if sh is None else sh
        hits = torch.empty((n,), dtype=torch.int32, device=dev) if hits is None else hits
        tmin = torch.empty((n,), dtype=torch.float32, device=dev) if tmin is None else tmin
        if cube is True:
            cube = torch.empty((n, 6, m, m, 3), dtype=torch.float32, device=dev)
        _ray_tensor("sh", sh, (n, 9, 3), torch.float32, dev)
        _ray_tensor("hits", hits, (n,), torch.int32, dev)
        _ray_tensor("tmin", tmin, (n,), torch.float32, dev)
        if cube is not None:
            _ray_tensor("cube", cube, (n, 6, m, m, 3), torch.float32, dev)
        p = ProbeParams.of(m, spp, max_bounce, seed, jitter, photon_maps, chunk_rays)
        sptr = self._stream_arg(stream, points)
        ptr = lambda a: None if a is None else (a.data_ptr() or None)   # noqa: E731
        if vis is None:
            _check(lib().qa_probe_sh_device(self._h, n, ptr(points), ptr(stream_ids), C.byref(p), ptr(sh), ptr(cube), ptr(hits), ptr(tmin), sptr))
        else:
            d = int(vis.d)
            if not 1 <= d <= m or m % d:
                raise ValueError(f"d: a divisor of m = {m} is expected, not {d}")
            moments = torch.empty((n, 6, d, d, 2), dtype=torch.float32, device=dev) if moments is None else moments
            _ray_tensor("moments", moments, (n, 6, d, d, 2), torch.float32, dev)
            _check(lib().qa_probevis_sh_device(self._h, n, ptr(points), ptr(stream_ids), C.byref(p), C.byref(vis), ptr(sh), ptr(cube), ptr(hits), ptr(tmin),
                                               ptr(moments), sptr))
        out = {"sh": sh, "hits": hits, "tmin": tmin}
        if cube is not None:
            out["cube"] = cube
        if vis is not None:
            out["moments"] = moments
        return out

    def probevis_sh_device(self, points, d=8, dmax=None, m=16, spp=1, max_bounce=5, seed=DEFAULT_SEED, jitter=False, photon_maps=False, stream_ids=None,
                           sh=None, cube=None, hits=None, tmin=None, chunk_rays=0, stream=None, moments=None):
        """qa_probevis_sh_device: probe_sh_device (its arguments, its outputs, their bits) and, from the same rays, the probes'
        distance moments for ProbeGrid.shade_device(visibility=True): moments float32 [n,6,d,d,2] (given, or allocated), a cube map
        of d x d cells per face (d divides m), each holding the mean of min(t, dmax) and of its square over the (m / d)^2 rays it
        pools; a miss counts as dmax, a void probe stores zeros.  dmax > 0 is the caller's: how far a probe needs to see (a grid
        takes 1.5 times its cell's diagonal).  No ray is traced beyond probe_sh_device's.  -> its dict and "moments".  Only
        enqueues."""
        if dmax is None:
            raise ValueError("dmax: how far a probe looks is expected (ProbeGrid.bake(visibility=True) takes 1.5 |spacing|)")
        return self._probe_sh_device(points, m, spp, max_bounce, seed, jitter, photon_maps, stream_ids, sh, cube, hits, tmin, chunk_rays, stream,
                                     ProbeVisParams.of(d, dmax), moments)

    def probe_sh(self, points, m=16, spp=1, max_bounce=5, seed=DEFAULT_SEED, jitter=False, photon_maps=False, stream_ids=None, cube=False,
                 chunk_rays=0):
        """qa_probe_sh: probe_sh_device from and to host memory.  points: [n,3], converted to float32; stream_ids: [n] integers below
        2^32 or None -> dict of numpy arrays sh [n,9,3] f32, hits [n] u32, tmin [n] f32, and cube [n,6,m,m,3] f32 with cube=True.
        Synchronises."""
        p = np.ascontiguousarray(points, dtype=np.float32)
        n = _ray_count("points", p)
        m = int(m)
        if not 1 <= m <= QA_PROBE_MAX_M:
            raise ValueError(f"m: 1 .. {QA_PROBE_MAX_M} is expected, not {m}")
        sid = None
        if stream_ids is not None:
            sid = np.ascontiguousarray(stream_ids, dtype=np.uint32)
            if sid.shape != (n,):
                raise ValueError(f"stream_ids: shape ({n},) is expected, not {sid.shape}")
        out = {"sh": np.zeros((n, 9, 3), np.float32), "hits": np.zeros(n, np.uint32), "tmin": np.zeros(n, np.float32)}
        if cube:
            out["cube"] = np.zeros((n, 6, m, m, 3), np.float32)
        par = ProbeParams.of(m, spp, max_bounce, seed, jitter, photon_maps, chunk_rays)
        _check(lib().qa_probe_sh(self._h, n, p.ctypes.data, _ptr(sid), C.byref(par), out["sh"].ctypes.data, _ptr(out.get("cube")), out["hits"].ctypes.data,
                                 out["tmin"].ctypes.data))
        return out

    def probevis_sh(self, points, d=8, dmax=None, m=16, spp=1, max_bounce=5, seed=DEFAULT_SEED, jitter=False, photon_maps=False, stream_ids=None,
                    cube=False, chunk_rays=0):
        """qa_probevis_sh: probevis_sh_device from and to host memory -> probe_sh's dict and moments [n,6,d,d,2] f32.  Synchronises."""
        if dmax is None:
            raise ValueError("dmax: how far a probe looks is expected (ProbeGrid.bake(visibility=True) takes 1.5 |spacing|)")
        p = np.ascontiguousarray(points, dtype=np.float32)
        n = _ray_count("points", p)
        m, d = int(m), int(d)
        if not 1 <= m <= QA_PROBE_MAX_M:
            raise ValueError(f"m: 1 .. {QA_PROBE_MAX_M} is expected, not {m}")
        if not 1 <= d <= m or m % d:
            raise ValueError(f"d: a divisor of m = {m} is expected, not {d}")
        sid = None
        if stream_ids is not None:
            sid = np.ascontiguousarray(stream_ids, dtype=np.uint32)
            if sid.shape != (n,):
                raise ValueError(f"stream_ids: shape ({n},) is expected, not {sid.shape}")
        out = {"sh": np.zeros((n, 9, 3), np.float32), "hits": np.zeros(n, np.uint32), "tmin": np.zeros(n, np.float32),
               "moments": np.zeros((n, 6, d, d, 2), np.float32)}
        if cube:
            out["cube"] = np.zeros((n, 6, m, m, 3), np.float32)
        par, vis = ProbeParams.of(m, spp, max_bounce, seed, jitter, photon_maps, chunk_rays), ProbeVisParams.of(d, dmax)
        _check(lib().qa_probevis_sh(self._h, n, p.ctypes.data, _ptr(sid), C.byref(par), C.byref(vis), out["sh"].ctypes.data, _ptr(out.get("cube")),
                                    out["hits"].ctypes.data, out["tmin"].ctypes.data, out["moments"].ctypes.data))
        return out

    def probe_shade_device(self, sh, normals, index=None, out=None, stream=None):
        """qa_probe_shade_device: the diffuse light of probes at shading points.  sh: float32 [probes,9,3] contiguous CUDA tensor
        (probe_sh_device's); normals: float32 [n,3], unit length; index: int32 [n] the probe of each shading point (None: point i
        takes probe i, probes >= n), an index outside [0, probes) is clamped into it -> out float32 [n,3] (given, or allocated) =
        max(0, sum_c A_c sh_c Y_c(N)): the units of irradiance_points_device, kd * out is a diffuse colour.  A normal that is not
        finite shades to 0.  Only enqueues."""
        import torch
        dev = torch.device("cuda", self.device_id)
        if not isinstance(sh, torch.Tensor):
            raise TypeError(f"sh: a torch tensor is expected, not {type(sh).__name__}")
        if sh.ndim != 3 or tuple(sh.shape[1:]) != (9, 3):
            raise ValueError(f"sh: shape (probes, 9, 3) is expected, not {tuple(sh.shape)}")
        probes = int(sh.shape[0])
        _ray_tensor("sh", sh, (probes, 9, 3), torch.float32, dev)
        if not isinstance(normals, torch.Tensor):
            raise TypeError(f"normals: a torch tensor is expected, not {type(normals).__name__}")
        n = _ray_count("normals", normals)
        _ray_tensor("normals", normals, (n, 3), torch.float32, dev)
        if index is not None:
            _ray_tensor("index", index, (n,), torch.int32, dev)
        elif probes < n:
            raise ValueError(f"sh: {n} probes are expected without an index, not {probes}")
        out = torch.empty((n, 3), dtype=torch.float32, device=dev) if out is None else out
        _ray_tensor("out", out, (n, 3), torch.float32, dev)
        sptr = self._stream_arg(stream, normals)
        ptr = lambda a: None if a is None else (a.data_ptr() or None)   # noqa: E731
        _check(lib().qa_probe_shade_device(self._h, n, ptr(sh), probes, ptr(normals), ptr(index), ptr(out), sptr))
        return out

    # -- reflection probes (qa_reflprobe.hip) ------------------------------------------------------
    def reflprobe_prefilter_device(self, cube, levels=None, chain=None, stream=None):
        """qa_reflprobe_prefilter_device: probe cubes prefiltered for glossy reflection.  cube: float32 [n,6,m,m,3] contiguous CUDA
        tensor (probe_sh_device's cube; m a power of two); levels: 1 .. log2 m + 1 (None: all, down to one texel per face) -> chain
        float32 [n,T,3] (given, or allocated; hip.reflprobe_layout says where each level lies): level 0 is the cube bit for bit,
        level l the cube at m >> l texels per face edge convolved with the Phong lobe of exponent 2^(2 (log2 m - l) - 1).  Reads and
        writes only these arrays and orders nothing: after probe_sh_device, pass its stream.  Only enqueues."""
        import torch
        dev = torch.device("cuda", self.device_id)
        if not isinstance(cube, torch.Tensor):
            raise TypeError(f"cube: a torch tensor is expected, not {type(cube).__name__}")
        if cube.ndim != 5 or tuple(cube.shape[1:2]) != (6,) or cube.shape[2] != cube.shape[3] or cube.shape[4] != 3:
            raise ValueError(f"cube: shape (n, 6, m, m, 3) is expected, not {tuple(cube.shape)}")
        n, m = int(cube.shape[0]), int(cube.shape[2])
        if n > QA_MAX_RAYS:
            raise ValueError("cube: more than 2^31 - 1 probes")
        lay = reflprobe_layout(m, levels)
        _ray_tensor("cube", cube, (n, 6, m, m, 3), torch.float32, dev)
        chain = torch.empty((n, lay["texels"], 3), dtype=torch.float32, device=dev) if chain is None else chain
        _ray_tensor("chain", chain, (n, lay["texels"], 3), torch.float32, dev)
        sptr = self._stream_arg(stream, cube)
        _check(lib().qa_reflprobe_prefilter_device(self._h, n, cube.data_ptr() or None, m, lay["levels"], chain.data_ptr() or None, sptr))
        return chain

    def reflprobe_shade_device(self, chain, m, dirs, level, levels=None, index=None, out=None, stream=None):
        """qa_reflprobe_shade_device: what a glossy surface sees in probes.  chain: float32 [probes,T,3] (reflprobe_prefilter_device's,
        of cubes of m x m texels with `levels` levels, None: all); dirs: float32 [n,3] the reflected directions, any length; level:
        float32 [n], clamped to [0, levels - 1] (hip.reflprobe_level gives it for a glossiness); index: int32 [n] the probe of each
        lookup (None: lookup i takes probe i, probes >= n), clamped into [0, probes) -> out float32 [n,3] (given, or allocated):
        bilinear inside the direction's face, linear between the two levels.  A direction that is zero or not finite, or a level
        that is NaN, gives 0.  Only enqueues."""
        import torch
        dev = torch.device("cuda", self.device_id)
        lay = reflprobe_layout(m, levels)
        if not isinstance(chain, torch.Tensor):
            raise TypeError(f"chain: a torch tensor is expected, not {type(chain).__name__}")
        if chain.ndim != 3 or tuple(chain.shape[1:]) != (lay["texels"], 3):
            raise ValueError(f"chain: shape (probes, {lay['texels']}, 3) is expected, not {tuple(chain.shape)}")
        probes = int(chain.shape[0])
        _ray_tensor("chain", chain, (probes, lay["texels"], 3), torch.float32, dev)
        if not isinstance(dirs, torch.Tensor):
            raise TypeError(f"dirs: a torch tensor is expected, not {type(dirs).__name__}")
        n = _ray_count("dirs", dirs)
        _ray_tensor("dirs", dirs, (n, 3), torch.float32, dev)
        _ray_tensor("level", level, (n,), torch.float32, dev)
        if index is not None:
            _ray_tensor("index", index, (n,), torch.int32, dev)
        elif probes < n:
            raise ValueError(f"chain: {n} probes are expected without an index, not {probes}")
        out = torch.empty((n, 3), dtype=torch.float32, device=dev) if out is None else out
        _ray_tensor("out", out, (n, 3), torch.float32, dev)
        sptr = self._stream_arg(stream, dirs)
        ptr = lambda a: None if a is None else (a.data_ptr() or None)   # noqa: E731
        _check(lib().qa_reflprobe_shade_device(self._h, n, ptr(chain), probes, int(m), lay["levels"], ptr(dirs), ptr(level), ptr(index), ptr(out), sptr))
        return out

    def camera_sample_rays_device(self, region, first=0, count=1, outputs=CAMERA_SAMPLE_OUTPUTS, stream=None, **given):
        """qa_camera_sample_rays_device: samples [first, first + count) of the camera rays of the pixels of a region, exactly as a
        frame builds them -> dict name -> CUDA tensor for the names in `outputs` (or the tensors passed by name): origins, dirs, dx,
        dy float32 [h*w,count,3], screen float32 [h*w,count,2] (the sample's position in pixels), stream_ids int32 [h*w] (y * width + x).
        radiance_rays_device(**them, spp=count) with first = 0 is render_region_device's frame bit for bit.  A camera with depth of
        field is refused (HipError, QA_EUNSUPPORTED).  Only enqueues."""
        import torch
        dev = torch.device("cuda", self.device_id)
        x0, y0, x1, y1 = (int(v) for v in region)
        first, count = int(first), int(count)
        n = max(x1 - x0, 0) * max(y1 - y0, 0)
        k = max(count, 0)
        shapes = {"origins": (n, k, 3), "dirs": (n, k, 3), "dx": (n, k, 3), "dy": (n, k, 3), "screen": (n, k, 2), "stream_ids": (n,)}
        for name in list(outputs) + list(given):
            if name not in shapes:
                raise ValueError(f"unknown output {name!r}: one of {CAMERA_SAMPLE_OUTPUTS}")
        out = {}
        for name in CAMERA_SAMPLE_OUTPUTS:
            dtype = torch.int32 if name == "stream_ids" else torch.float32
            if given.get(name) is not None:
                out[name] = _ray_tensor(name, given[name], shapes[name], dtype, dev)
            elif name in outputs and name not in given:
                out[name] = torch.empty(shapes[name], dtype=dtype, device=dev)
        if not out:
            raise ValueError("no output asked for")
        sptr = self._stream_arg(stream, next(iter(out.values())))
        _check(lib().qa_camera_sample_rays_device(self._h, x0, y0, x1, y1, first, count,
                                                  *((out[name].data_ptr() or None) if name in out else None for name in CAMERA_SAMPLE_OUTPUTS), sptr))
        return out

    def camera_sample_rays(self, region, first=0, count=1, outputs=CAMERA_SAMPLE_OUTPUTS):
        """camera_sample_rays_device to host memory -> dict name -> numpy array.  Synchronises."""
        out = self.camera_sample_rays_device(region, first, count, outputs)
        self.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}

    def render_strips_device(self, region, first_strip, strip_step, spp, rgb, depth, ns, max_bounce=5,
                             seed=DEFAULT_SEED, spp_max=None, stats=False, stream=None):
        """Render strips first_strip, first_strip+strip_step, ... (8 rows each) of `region` into PACKED
        torch CUDA tensors of strip_count(...)*8 rows."""
        x0, y0, x1, y1 = region
        n = strip_count(y0, y1, first_strip, strip_step) * 8 * (x1 - x0)
        assert rgb.is_cuda and rgb.is_contiguous() and rgb.numel() == 3 * n and rgb.element_size() == 4
        assert depth.is_cuda and depth.is_contiguous() and depth.numel() == n and depth.element_size() == 4
        assert ns.is_cuda and ns.is_contiguous() and ns.numel() == n and ns.element_size() == 4
        spp_max = spp if spp_max is None else spp_max
        sptr = self._stream_arg(stream, rgb)
        _check(lib().qa_render_strips_device(self._h, x0, y0, x1, y1, first_strip, strip_step, spp, spp_max,
                                             max_bounce, seed, QA_RENDER_STATS if stats else 0, rgb.data_ptr(),
                                             depth.data_ptr(), ns.data_ptr(), sptr))

    def empty_tiles_device(self, region, mask, first_strip=0, strip_step=1, stream=None):
        """qa_empty_tiles_device: which 8x8 tiles of such a launch the frame finishes in closed form, because no camera ray of theirs
        can hit anything (option 'empty_tiles': rgb = background, depth = 1e30, ns = spp_min, samples derived and not traced) - the
        decision of the frame's kernel, by the same device function, into `mask`, a torch CUDA uint8 tensor of
        strip_count(...) * ((x1 - x0 + 7) // 8) elements (1 = empty).  All zero where a frame of this context takes no such decision
        (another kernel, the option off, depth of field, tile lists off).  Only enqueues."""
        x0, y0, x1, y1 = (int(v) for v in region)
        n = strip_count(y0, y1, first_strip, strip_step) * ((x1 - x0 + 7) // 8)
        assert mask.is_cuda and mask.is_contiguous() and mask.numel() == n and mask.element_size() == 1
        sptr = self._stream_arg(stream, mask)
        _check(lib().qa_empty_tiles_device(self._h, x0, y0, x1, y1, int(first_strip), int(strip_step), mask.data_ptr(), sptr))

    def empty_tiles(self, region, first_strip=0, strip_step=1):
        """empty_tiles_device to host memory -> bool [strips, tiles per strip].  Synchronises."""
        import torch
        x0, y0, x1, y1 = (int(v) for v in region)
        shape = (strip_count(y0, y1, first_strip, strip_step), (x1 - x0 + 7) // 8)
        mask = torch.zeros(shape, dtype=torch.uint8, device=torch.device("cuda", self.device_id))
        self.empty_tiles_device(region, mask, first_strip, strip_step)
        self.synchronize()
        return mask.cpu().numpy().astype(bool)

    @staticmethod
    def _stream_arg(stream, tensor):
        """No stream given: the render runs on the context's own non-blocking stream, which is not ordered against
        torch's streams - so first wait for whatever torch has queued on the tensor's device (e.g. the zero-fill of
        freshly created output tensors).  The caller still has to synchronize() before reading the outputs."""
        if stream:
            return C.c_void_p(stream)
        import torch
        torch.cuda.current_stream(tensor.device).synchronize()
        return None

    def synchronize(self):
        _check(lib().qa_synchronize(self._h))

    def request_stop(self):
        _check(lib().qa_request_stop(self._h))

    def clear_stop(self):
        _check(lib().qa_clear_stop(self._h))

    # -- measurement ---------------------------------------------------------------------------
    def counters(self):
        c = Counters()
        _check(lib().qa_get_counters(self._h, C.byref(c)))
        return c.as_dict()

    def reset_counters(self):
        _check(lib().qa_reset_counters(self._h))

    def kernel_time(self):
        """-> (total_ms, launches) of the integrator kernel since the last reset (HIP events)."""
        ms, n = C.c_double(), C.c_uint64()
        _check(lib().qa_get_kernel_time(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    PIPELINES = {"mega": 0, "staged": 1, "auto": 2}

    def set_pipeline(self, mode):
        """'mega' | 'staged' | 'auto' (= mega): which integrator renders scenes that do not fit LDS (same bits either way)."""
        _check(lib().qa_set_pipeline(self._h, self.PIPELINES[mode]))

    def set_option(self, name, value):
        """qa_set_option: 'coop', 'cs_cull', 'cs_force_exact', 'walk_zero_terms', 'cs_pool_limit', 'chunk_spp', 'chunk_tail', 'tile_lists', 'last_cast', 'leaf_sweep', 'empty_tiles', 'sync_samples', 'tile_order', 'staged_groups', 'verbose',
        'progressive_tile_limit'."""
        _check(lib().qa_set_option(self._h, name.encode(), int(value)))

    def kernel_name(self):
        """The integrator the uploaded scene runs on (megakernel variant or the staged pipeline)."""
        return lib().qa_get_kernel_name(self._h).decode()

    STAGED_FIELDS = ("passes", "rays_closest", "rays_shadow", "jobs_queued", "rays_redone", "jobs_done", "node_steps", "leaf_steps",
                     "tri_tests", "order_check_failed", "jobs_suspended", "lane_slots", "wave_rounds")

    def staged_stats(self):
        """Diagnostics of the staged integrator since the last reset_counters()."""
        v = (C.c_uint64 * len(self.STAGED_FIELDS))()
        _check(lib().qa_get_staged_stats(self._h, v))
        d = {k: int(x) for k, x in zip(self.STAGED_FIELDS, v)}
        d["lane_utilisation"] = d["lane_slots"] / (64.0 * d["wave_rounds"]) if d["wave_rounds"] else 0.0
        d["geometry_bytes"] = d["node_steps"] * 64 + d["tri_tests"] * 48
        return d

    def reset_kernel_time(self):
        _check(lib().qa_reset_kernel_time(self._h))

    def scrub_scratch(self, pattern):
        """qa_debug_scrub_scratch: every wave slot's private segment filled with `pattern` (tests: frames must not depend on it)."""
        _check(lib().qa_debug_scrub_scratch(self._h, pattern & 0xFFFFFFFF))

    def set_launch_config(self, blocks_per_cu=0, threads_per_block=0):
        _check(lib().qa_set_launch_config(self._h, blocks_per_cu, threads_per_block))

    def close(self):
        if self._h:
            lib().qa_ctx_destroy(self._h)   # (waits for the context's stream)
            self._h = C.c_void_p()
            self._tmax_fill = None
            self._bake_stream = None   # (bake_ao's side stream)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Progressive:
    """A progressive frame of a Context (Context.progressive).  advance() enqueues a pass, read() returns the preview
    (finished pixels' final values, the running mean and samples so far of the others), status() how far it got."""

    def __init__(self, ctx, region):
        self._ctx = ctx
        self.region = tuple(region)

    def advance(self, spp_target, stream=None):
        """Bring every unfinished pixel to min(spp_target, spp_max) samples (one megakernel launch, enqueued on `stream`,
        a HIP stream handle; None = the context's own stream)."""
        _check(lib().qa_progressive_advance(self._ctx._h, int(spp_target), C.c_void_p(stream) if stream else None))

    @property
    def tile_shape(self):
        """(tiles_y, tiles_x) of the region's 8x8 tiles (qa_progressive_tile_count): the shape of every per-tile array."""
        x0, y0, x1, y1 = self.region
        return (y1 - y0 + 7) // 8, (x1 - x0 + 7) // 8

    def _tile_tensor(self, out, dtype, what):
        """The (ty, tx) CUDA tensor of a per-tile device call, checked (or made where it is None)."""
        import torch
        device = torch.device("cuda", self._ctx.device_id)
        if out is None:
            return torch.empty(self.tile_shape, dtype=dtype, device=device)
        if not isinstance(out, torch.Tensor):
            raise TypeError(f"{what}: a torch tensor is expected")
        if not out.is_cuda or out.device != device:
            raise ValueError(f"{what}: the tensor must be on {device}")
        if out.dtype != dtype or tuple(out.shape) != self.tile_shape:
            raise ValueError(f"{what}: {dtype} of shape {self.tile_shape} is expected, not {out.dtype} {tuple(out.shape)}")
        if not out.is_contiguous():
            raise ValueError(f"{what}: the tensor must be contiguous")
        return out

    def advance_tiles(self, spp_target, tiles, stream=None):
        """qa_progressive_advance_tiles[_device]: advance(spp_target) for the selected tiles alone.  tiles: a numpy bool / uint8
        array of tile_shape, or a torch uint8 tensor of that shape on the context's device, which must stay as it is until the
        pass has run; non-zero = selected.  Only enqueues; a later advance(spp_target) completes the other tiles."""
        if isinstance(tiles, np.ndarray):
            if tiles.dtype not in (np.bool_, np.uint8):
                raise TypeError(f"tiles: bool or uint8 is expected, not {tiles.dtype}")
            if tiles.shape != self.tile_shape:
                raise ValueError(f"tiles: shape {self.tile_shape} is expected, not {tiles.shape}")
            mask = np.ascontiguousarray(tiles).view(np.uint8)
            _check(lib().qa_progressive_advance_tiles(self._ctx._h, int(spp_target), mask.ctypes.data, C.c_void_p(stream) if stream else None))
            return
        import torch
        tiles = self._tile_tensor(tiles, torch.uint8, "tiles")
        _check(lib().qa_progressive_advance_tiles_device(self._ctx._h, int(spp_target), tiles.data_ptr(), Context._stream_arg(stream, tiles)))

    def tile_levels(self):
        """qa_progressive_tile_levels -> uint32 array of tile_shape: the samples every unfinished pixel of a tile has; synchronises."""
        out = np.zeros(self.tile_shape, np.uint32)
        _check(lib().qa_progressive_tile_levels(self._ctx._h, out.ctypes.data))
        return out

    def tile_error(self):
        """qa_progressive_tile_error -> float32 array of tile_shape: the estimated variance of the tiles' pixel means (+inf before a
        live pixel's second sample, 0 where all are finished); frames begun with spp < spp_max only.  Synchronises."""
        out = np.zeros(self.tile_shape, np.float32)
        _check(lib().qa_progressive_tile_error(self._ctx._h, out.ctypes.data))
        return out

    def tile_levels_device(self, out=None, stream=None):
        """qa_progressive_tile_levels_device: tile_levels() into a torch CUDA tensor (int32 of tile_shape; None: a new one) -> out;
        only enqueues."""
        import torch
        out = self._tile_tensor(out, torch.int32, "out")
        _check(lib().qa_progressive_tile_levels_device(self._ctx._h, out.data_ptr(), Context._stream_arg(stream, out)))
        return out

    def tile_error_device(self, out=None, stream=None):
        """qa_progressive_tile_error_device: tile_error() into a torch CUDA tensor (float32 of tile_shape; None: a new one) -> out;
        only enqueues."""
        import torch
        out = self._tile_tensor(out, torch.float32, "out")
        _check(lib().qa_progressive_tile_error_device(self._ctx._h, out.data_ptr(), Context._stream_arg(stream, out)))
        return out

    def advance_adaptive(self, spp_target, max_tiles=0, fraction=None, min_error=0.0, stream=None):
        """qa_progressive_advance_adaptive: advance(spp_target) for the noisiest tiles alone - of the tiles below the target whose
        error exceeds min_error, the max_tiles of greatest error (0: all of them), or `fraction` of the frame's tiles (rounded up,
        at least one).  Chosen on the device, only enqueues; adaptive_info() says afterwards how many were taken."""
        if fraction is not None:
            if max_tiles:
                raise ValueError("max_tiles and fraction exclude each other")
            if not 0.0 < fraction <= 1.0:
                raise ValueError("fraction must be in (0, 1]")
            ty, tx = self.tile_shape
            max_tiles = max(1, int(np.ceil(fraction * (ty * tx))))
        if max_tiles < 0 or max_tiles > 0xFFFFFFFF:
            raise ValueError("max_tiles out of range")
        if not min_error >= 0.0:
            raise ValueError("min_error must not be negative or a NaN")
        _check(lib().qa_progressive_advance_adaptive(self._ctx._h, int(spp_target), int(max_tiles), float(min_error),
                                                     C.c_void_p(stream) if stream else None))

    def adaptive_info(self):
        """qa_progressive_adaptive_info -> dict of the last adaptive pass: selected, candidates, cut_error and max_finite_error
        (floats; 0.0: none); synchronises."""
        v = (C.c_uint64 * 4)()
        _check(lib().qa_progressive_adaptive_info(self._ctx._h, v))
        bits = np.array([v[2], v[3]], np.uint32).view(np.float32)
        return {"selected": int(v[0]), "candidates": int(v[1]), "cut_error": float(bits[0]), "max_finite_error": float(bits[1])}

    def state(self):
        """qa_progressive_state -> uint32 [h,w,8]: every pixel's RNG state, samples taken | bit 31 finished, running mean (3 float
        words) and variance (3); synchronises."""
        x0, y0, x1, y1 = self.region
        out = np.zeros((y1 - y0, x1 - x0, 8), np.uint32)
        _check(lib().qa_progressive_state(self._ctx._h, out.ctypes.data))
        return out

    def read(self):
        """-> (rgb[h,w,3] f32, depth[h,w] f32, ns[h,w] u32), as render_region returns them; synchronises."""
        x0, y0, x1, y1 = self.region
        h, w = y1 - y0, x1 - x0
        rgb = np.zeros((h, w, 3), np.float32)
        depth = np.zeros((h, w), np.float32)
        ns = np.zeros((h, w), np.uint32)
        _check(lib().qa_progressive_read(self._ctx._h, rgb.ctypes.data, depth.ctypes.data, ns.ctypes.data))
        return rgb, depth, ns

    def read_device(self, rgb, depth, ns, stream=None):
        """The preview into torch CUDA tensors (float32 [h,w,3], float32 [h,w], int32/uint32 [h,w]); only enqueues (see
        Context.render_region_device for the stream)."""
        x0, y0, x1, y1 = self.region
        n = (x1 - x0) * (y1 - y0)
        assert rgb.is_cuda and rgb.is_contiguous() and rgb.numel() == 3 * n and rgb.element_size() == 4
        assert depth.is_cuda and depth.is_contiguous() and depth.numel() == n and depth.element_size() == 4
        assert ns.is_cuda and ns.is_contiguous() and ns.numel() == n and ns.element_size() == 4
        sptr = Context._stream_arg(stream, rgb)
        _check(lib().qa_progressive_read_device(self._ctx._h, rgb.data_ptr(), depth.data_ptr(), ns.data_ptr(), sptr))

    def display(self, srgb=True):
        """qa_progressive_display: the frame's 8-bit products as the host FrameBuffer would make them of read(), computed on
        the device from the frame's own slabs (7 bytes per pixel come back) -> Display(color[h,w,3], count, zimg, countimg,
        mask [h,w] uint8, stats dict); synchronises."""
        x0, y0, x1, y1 = self.region
        h, w = y1 - y0, x1 - x0
        out = [np.zeros((h, w, 3) if k == 0 else (h, w), np.uint8) for k in range(5)]
        st = DisplayStats()
        _check(lib().qa_progressive_display(self._ctx._h, int(bool(srgb)), *(a.ctypes.data for a in out), C.byref(st)))
        return Display(*out, st.as_dict())

    def display_device(self, srgb=True, stream=None, want=DISPLAY_ALL, **given):
        """qa_progressive_display_device: the same products into torch CUDA tensors on the context's device (see
        Context.display_device for want / given and the result); only enqueues."""
        import torch
        device = torch.device("cuda", self._ctx.device_id)
        x0, y0, x1, y1 = self.region
        out, ptrs = _display_outputs((x1 - x0) * (y1 - y0), device, want, given)
        if stream:
            sptr = C.c_void_p(stream)
        else:
            torch.cuda.current_stream(device).synchronize()
            sptr = None
        _check(lib().qa_progressive_display_device(self._ctx._h, int(bool(srgb)), *ptrs, sptr))
        return out

    def _denoise_out(self, out=None, tensor=False):
        """The float32 [h,w,3] output of the four denoise* calls: a new numpy array, or (tensor) out checked, a new CUDA tensor on the
        context's device where it is None."""
        x0, y0, x1, y1 = self.region
        if not tensor:
            return np.zeros((y1 - y0, x1 - x0, 3), np.float32)
        import torch
        if out is None:
            out = torch.empty((y1 - y0, x1 - x0, 3), dtype=torch.float32, device=torch.device("cuda", self._ctx.device_id))
        assert out.is_cuda and out.is_contiguous() and out.numel() == 3 * (x1 - x0) * (y1 - y0) and out.dtype == torch.float32
        return out

    def denoise(self, params=None, iterations=None, sigma_color=None, sigma_depth=None):
        """qa_progressive_denoise: the preview read() returns, filtered on the device straight from the frame's slabs (see
        Context.denoise_device) -> rgb[h,w,3] f32; synchronises.  The frame is not changed."""
        rgb = self._denoise_out()
        p = DenoiseParams.of(params, iterations, sigma_color, sigma_depth)
        _check(lib().qa_progressive_denoise(self._ctx._h, C.byref(p), rgb.ctypes.data))
        return rgb

    def denoise_device(self, out=None, params=None, iterations=None, sigma_color=None, sigma_depth=None, stream=None):
        """qa_progressive_denoise_device: the same into a torch CUDA tensor (float32 [h,w,3]; None: a new one) on the context's
        device -> out; only enqueues."""
        out = self._denoise_out(out, tensor=True)
        p = DenoiseParams.of(params, iterations, sigma_color, sigma_depth)
        _check(lib().qa_progressive_denoise_device(self._ctx._h, C.byref(p), out.data_ptr(), Context._stream_arg(stream, out)))
        return out

    def denoise_guided(self, params=None, flags=None, iterations=None, sigma_color=None, sigma_depth=None, sigma_normal=None):
        """qa_progressive_denoise_guided: denoise() guided by the frame's own first-hit planes, which the call computes from the scene
        as it now stands (flags: which guides; default both) -> rgb[h,w,3] f32; synchronises.  The frame is not changed."""
        rgb = self._denoise_out()
        p = DenoiseGuidedParams.of(params, flags, iterations, sigma_color, sigma_depth, sigma_normal)
        _check(lib().qa_progressive_denoise_guided(self._ctx._h, C.byref(p), rgb.ctypes.data))
        return rgb

    def denoise_guided_device(self, out=None, params=None, flags=None, iterations=None, sigma_color=None, sigma_depth=None, sigma_normal=None,
                              stream=None):
        """qa_progressive_denoise_guided_device: the same into a torch CUDA tensor (float32 [h,w,3]; None: a new one) -> out; only
        enqueues."""
        out = self._denoise_out(out, tensor=True)
        p = DenoiseGuidedParams.of(params, flags, iterations, sigma_color, sigma_depth, sigma_normal)
        _check(lib().qa_progressive_denoise_guided_device(self._ctx._h, C.byref(p), out.data_ptr(), Context._stream_arg(stream, out)))
        return out

    def gbuffer_device(self, normal=None, albedo=None, depth=None, ids=None, stream=None):
        """qa_progressive_gbuffer_device: the guide planes of the frame's region and seed, of the scene as it now stands (see
        Context.gbuffer_device) -> dict name -> tensor; only enqueues."""
        import torch
        out, ptrs = _output_tensors(GBUFFER_PLANES, *_region_planes(self.region, GBUFFER_PLANES), torch.device("cuda", self._ctx.device_id),
                                    dict(normal=normal, albedo=albedo, depth=depth, ids=ids))
        sptr = Context._stream_arg(stream, next(iter(out.values())))
        _check(lib().qa_progressive_gbuffer_device(self._ctx._h, *ptrs, sptr))
        return out

    def matte_device(self, coverage=None, albedo=None, normal=None, backdrop=None, stream=None):
        """qa_progressive_matte_device: the matte planes of the frame's region over the samples each pixel holds now, of the scene as
        it now stands (see Context.matte_device: its planes for spp_max and the ns plane read() gives) -> dict name -> tensor; only
        enqueues."""
        import torch
        out, ptrs = _output_tensors(MATTE_PLANES, *_region_planes(self.region, MATTE_PLANES), torch.device("cuda", self._ctx.device_id),
                                    dict(coverage=coverage, albedo=albedo, normal=normal, backdrop=backdrop))
        sptr = Context._stream_arg(stream, next(iter(out.values())))
        _check(lib().qa_progressive_matte_device(self._ctx._h, *ptrs, sptr))
        return out

    def idmatte_device(self, key="node", ids=None, counts=None, other=None, samples=None, stream=None):
        """qa_progressive_idmatte_device: the id matte of the frame's region over the samples each pixel holds now, of the scene as it
        now stands (see Context.idmatte_device: its planes for spp_max and the ns plane read() gives) -> dict name -> tensor; only
        enqueues."""
        import torch
        out, ptrs = _output_tensors(IDMATTE_PLANES, *_idmatte_planes(self.region), torch.device("cuda", self._ctx.device_id),
                                    dict(ids=ids, counts=counts, other=other, samples=samples))
        sptr = Context._stream_arg(stream, next(iter(out.values())))
        _check(lib().qa_progressive_idmatte_device(self._ctx._h, _idmatte_key(key), *ptrs, sptr))
        return out

    def ao_device(self, K=4, radius=float("inf"), open=None, rays=None, ao=None, stream=None):
        """qa_progressive_ao_device: the ambient occlusion of the frame's region over the samples each pixel holds now, with the
        frame's seed, of the scene as it now stands (see Context.ao_device: its planes for first 0, spp_max and the ns plane read()
        gives) -> dict name -> tensor; only enqueues."""
        import torch
        out, ptrs = _output_tensors(AO_PLANES, *_ao_planes(self.region), torch.device("cuda", self._ctx.device_id), dict(open=open, rays=rays, ao=ao))
        sptr = Context._stream_arg(stream, next(iter(out.values())))
        _check(lib().qa_progressive_ao_device(self._ctx._h, int(K), float(radius), *ptrs, sptr))
        return out

    def reproject_device(self, history, prev_cam, hist_ids=None, out=None, out_length=None, params=None, depth_tolerance=None, max_history=None,
                         stream=None):
        """qa_progressive_reproject_device: Context.reproject_device with the frame's preview (the floats read() returns, straight
        from its slabs), its region and the resident scene's camera as the current frame; history = (rgb, depth, length) torch CUDA
        tensors accumulated under prev_cam.  With hist_ids (int32 [h,w,2]) the frame's own ids are computed as gbuffer_device does.
        -> (out, out_length); only enqueues.  The frame is not changed; a stale frame (after an edit) wants restart() first."""
        _, _, head, keep, out, out_length = _reproject_progressive_planes(self, history, prev_cam, hist_ids, out, out_length)
        p = ReprojectParams.of(params, depth_tolerance, max_history)
        sptr = Context._stream_arg(stream, out)
        _check(lib().qa_progressive_reproject_device(*head, C.byref(p), _ptr(out), _ptr(out_length), sptr))
        return out, out_length

    def reproject_motion_device(self, history, prev_cam, hist_ids=None, motion=None, out=None, out_length=None, params=None, depth_tolerance=None,
                                max_history=None, clamp=None, clamp_radius=None, clamp_gamma=None, stream=None):
        """qa_progressive_reproject_motion_device: reproject_device of this frame with Context.reproject_motion_device's additions
        (motion: a numpy table or a CUDA tensor, wants hist_ids; clamp, clamp_radius, clamp_gamma).  -> (out, out_length); only
        enqueues.  The frame is not changed; a stale frame wants restart() first."""
        _, device, head, keep, out, out_length = _reproject_progressive_planes(self, history, prev_cam, hist_ids, out, out_length)
        table, count = self._ctx._upload_motion(motion, device, stream)
        p = ReprojectMotionParams.of(params, depth_tolerance, max_history, True if motion is not None else None, clamp, clamp_radius, clamp_gamma)
        sptr = Context._stream_arg(stream, out)
        _check(lib().qa_progressive_reproject_motion_device(*head, table, count, C.byref(p), _ptr(out), _ptr(out_length), sptr))
        return out, out_length

    def reproject_moments_device(self, history, prev_cam, hist_ids=None, hist_moments=None, motion=None, out=None, out_length=None, out_moments=None,
                                 out_variance=None, params=None, depth_tolerance=None, max_history=None, clamp=None, clamp_radius=None, clamp_gamma=None,
                                 moments=None, shorten=None, min_frames=None, shorten_rate=None, stream=None):
        """qa_progressive_reproject_moments_device: reproject_motion_device of this frame with Context.reproject_moments_device's
        additions (hist_moments, moments, shorten, min_frames, shorten_rate).  -> (out, out_length, out_moments, out_variance); only
        enqueues.  The frame is not changed; a stale frame wants restart() first."""
        (h, w), device, head, keep, out, out_length = _reproject_progressive_planes(self, history, prev_cam, hist_ids, out, out_length)
        p = ReprojectMomentsParams.of(params, depth_tolerance, max_history, True if motion is not None else None, clamp, clamp_radius, clamp_gamma,
                                      moments, shorten, min_frames, shorten_rate)
        out_moments, out_variance = _moments_tensors(p, h, w, device, hist_moments, out_moments, out_variance)
        table, count = self._ctx._upload_motion(motion, device, stream)
        sptr = Context._stream_arg(stream, out)
        _check(lib().qa_progressive_reproject_moments_device(*head, _ptr(hist_moments), table, count, C.byref(p), _ptr(out), _ptr(out_length),
                                                             _ptr(out_moments), _ptr(out_variance), sptr))
        return out, out_length, out_moments, out_variance

    def status(self):
        """-> dict(spp_reached, pixels_finished, tiles_behind); synchronises."""
        r, f, b = C.c_int(), C.c_uint64(), C.c_uint64()
        _check(lib().qa_progressive_status(self._ctx._h, C.byref(r), C.byref(f), C.byref(b)))
        return {"spp_reached": r.value, "pixels_finished": f.value, "tiles_behind": b.value}

    def restart(self):
        """qa_progressive_restart: the same frame from level 0 again (after a scene edit); nothing is freed or allocated."""
        _check(lib().qa_progressive_restart(self._ctx._h))

    def close(self):
        """End the frame (qa_progressive_end) unless a newer frame of the context has replaced it."""
        if self._ctx is not None and self._ctx._h and getattr(self._ctx, "_prog", None) is self:
            _check(lib().qa_progressive_end(self._ctx._h))
            self._ctx._prog = None
        self._ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


class TemporalPreview:
    """The history of an interactive preview across camera moves, node moves and scene edits: torch plumbing around
    Context.reproject_device and Context.reproject_motion_device.  Owns the accumulated colour and length (two of each: a call reads
    one and writes the other), the depth and ids of the last frame, the last camera and the last instance table.
        tp = TemporalPreview(ctx, region, clamp=True)
        per frame: ctx.edit_camera(cam) / ctx.edit_instances(first, records) / ctx.edit_lights(...)
                   ctx.render_region_device(region, 4, rgb, depth, ns, seed=NEW SEED, stream=s)
                   g = ctx.gbuffer_device(region, seed, ids=ids, stream=s)
                   acc, length = tp.push(cam, rgb, depth, ns, ids, instances=TABLE AS IT NOW STANDS, stream=s)
    A new seed per frame matters: frames of one seed repeat their noise, and accumulating them gains nothing.
    With instances= (and ids) on every push, node moves (edit_instances) need no reset: the history follows the node.  With
    clamp=True, light, material and texture edits need no reset: the history is clamped to the current frame's neighbourhood and
    leaves within a few frames.  reset() is still needed after an edit that changes ids or topology (a new scene upload), and after
    any edit that is not a camera move when neither of the two is in use (include/qaray_hip.h).
    With shorten=True (wants clamp=True) a history the clamp moved also loses its length, so the frames after an edit stop weighing
    it.  With moments=True the preview also carries the luma's moments: tp.variance is then the plane of the last push (float32
    [h,w], the variance of the accumulated colour's luma, -1 where there is none - everywhere after the first push and after
    reset()), and None before the first push or without moments.  With both off a push makes the calls it made before."""

    def __init__(self, ctx, region, params=None, depth_tolerance=None, max_history=None, clamp=False, clamp_radius=None, clamp_gamma=None,
                 moments=False, shorten=False, min_frames=None, shorten_rate=None):
        import torch
        self._ctx = ctx
        self.region = tuple(region)
        x0, y0, x1, y1 = self.region
        h, w = y1 - y0, x1 - x0
        dev = torch.device("cuda", ctx.device_id)
        self.params = ReprojectParams.of(params, depth_tolerance, max_history)
        self.motion_params = ReprojectMotionParams.of(None, self.params.depth_tolerance, self.params.max_history, None, bool(clamp), clamp_radius,
                                                      clamp_gamma)
        self._rgb = [torch.zeros((h, w, 3), dtype=torch.float32, device=dev) for _ in range(2)]
        self._length = [torch.zeros((h, w), dtype=torch.float32, device=dev) for _ in range(2)]
        self._depth = torch.zeros((h, w), dtype=torch.float32, device=dev)
        self._ids = torch.zeros((h, w, 2), dtype=torch.int32, device=dev)
        self._has_ids = False
        self._cam = None
        self._instances = None
        self._at = 0
        # moments / shorten: every push goes through reproject_moments_device, which owns two moment planes and a variance plane
        self.moments_params = None
        self.variance = None
        if moments or shorten:
            self.moments_params = ReprojectMomentsParams.of(None, self.params.depth_tolerance, self.params.max_history, None, bool(clamp),
                                                            self.motion_params.clamp_radius, self.motion_params.clamp_gamma, bool(moments), bool(shorten),
                                                            min_frames, shorten_rate)
        if moments:
            self._moments = [torch.zeros((h, w, 2), dtype=torch.float32, device=dev) for _ in range(2)]
            self._variance = torch.full((h, w), -1.0, dtype=torch.float32, device=dev)
        torch.cuda.current_stream(dev).synchronize()

    def reset(self):
        """Forget the history: the next push returns its frame as it is."""
        self._cam = None
        self._instances = None

    def push(self, cam, rgb, depth, ns, ids=None, instances=None, stream=None):
        """The frame (rgb, depth, ns[, ids]: torch CUDA tensors as render_region_device and gbuffer_device fill them) rendered from
        cam (a record of CAMERA_DTYPE) joins the history -> (accumulated rgb float32 [h,w,3], length float32 [h,w]); the first push,
        and one after reset(), returns the frame itself with length = ns.  The ids are compared when this push and the last one
        both brought them.  instances: the scene's whole INSTANCE_DTYPE table as it stands for this frame
        (blob_table(ctx.download_scene(), "instances"), or the caller's own edited copy; it is copied); when this push and the last
        one both brought instances and ids, the history of a node that moved in between is fetched from where the node was
        (node_motion).  The two tensors returned are the preview's own and stay as they are until the push after the next one.
        The caller's tensors are free again when the call returns (depth and ids are copied).  stream: the HIP stream handle the
        frame was rendered on: everything is enqueued there.  None: the frame was rendered on the context's own stream, and the
        call synchronises (see render_region_device)."""
        import torch
        dev = self._depth.device
        cam = _camera_record(cam)
        if instances is not None:
            instances = np.array(instances, dtype=INSTANCE_DTYPE).reshape(-1)
        if stream:
            ts = torch.cuda.ExternalStream(stream, device=dev)
        else:
            self._ctx.synchronize()
            ts = torch.cuda.current_stream(dev)
        prev, nxt = self._at, 1 - self._at
        fresh = self._cam is None
        if fresh:
            with torch.cuda.stream(ts):
                self._length[prev].zero_()   # no history anywhere: the kernel hands the frame through
        with_ids = ids is not None and self._has_ids and not fresh
        motion = None
        if with_ids and instances is not None and self._instances is not None:
            motion = node_motion(self._instances, instances)
        x0, y0 = self.region[:2]
        frame, history = (rgb, depth, ns), (self._rgb[prev], self._depth, self._length[prev])
        kw = dict(origin=(x0, y0), ids=ids if with_ids else None, hist_ids=self._ids if with_ids else None, out=self._rgb[nxt],
                  out_length=self._length[nxt], stream=stream)
        if self.moments_params is not None:
            with_moments = bool(self.moments_params.flags & QA_REPROJECT_MOMENTS)
            if with_moments:   # (a fresh history has length 0 everywhere: no tap counts, and the stale moments are not read)
                kw.update(hist_moments=self._moments[prev], out_moments=self._moments[nxt], out_variance=self._variance)
            self._ctx.reproject_moments_device(frame, history, cam if fresh else self._cam, cam, motion=motion, params=self.moments_params, **kw)
            if with_moments:
                self.variance = self._variance
        elif motion is None and not self.motion_params.flags:
            self._ctx.reproject_device(frame, history, cam if fresh else self._cam, cam, params=self.params, **kw)
        else:
            self._ctx.reproject_motion_device(frame, history, cam if fresh else self._cam, cam, motion=motion, params=self.motion_params, **kw)
        if not stream:
            self._ctx.synchronize()
        with torch.cuda.stream(ts):
            self._depth.view(-1).copy_(depth.reshape(-1))
            if ids is not None:
                self._ids.view(-1).copy_(ids.reshape(-1))
        if not stream:
            ts.synchronize()
        self._has_ids = ids is not None
        self._instances = instances
        self._cam = cam
        self._at = nxt
        return self._rgb[nxt], self._length[nxt]


class ProbeGrid:
    """A regular grid of light probes over a Context's scene: probe (iz * ny + iy) * nx + ix stands at origin + (ix, iy, iz) *
    spacing.  bake() traces and projects them (Context.probe_sh_device) and keeps sh, hits and tmin on the device; shade_device()
    gives the diffuse light at any points from the trilinearly interpolated coefficients - what a viewer asks for the nodes it
    moves with edit_instances.  hits and tmin tell which probes sit inside a wall or against one.  bake(visibility=True) also keeps
    the probes' distance moments, and shade_device(visibility=True) then weighs each probe by whether it can see the point, so
    that a wall between them stops the light.  bake(reflections=True) also keeps the probes' prefiltered cube chains,
    and reflect_device() gives what a glossy surface at a point sees in a direction."""

    def __init__(self, ctx, origin, spacing, counts):
        self.ctx = ctx
        self.origin, self.spacing, self.counts = _probe_grid_args(origin, spacing, counts)
        if not (np.isfinite(self.origin).all() and np.isfinite(self.spacing).all() and (self.spacing > 0).all() and (self.counts >= 1).all()):
            raise ValueError("a grid has a finite origin, spacing > 0 and counts >= 1")
        self.probes = int(np.prod(self.counts.astype(np.int64)))
        if self.probes > QA_MAX_RAYS:
            raise ValueError("more than 2^31 - 1 probes")
        self.sh = self.hits = self.tmin = self.moments = self.d = self.dmax = self.chain = self.m = self.levels = None

    def points(self):
        """-> the probes' positions, float32 (nz * ny * nx, 3) numpy, in the grid's order: origin + (ix, iy, iz) * spacing in fp32"""
        nx, ny, nz = (int(v) for v in self.counts)
        iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
        idx = np.stack([ix, iy, iz], axis=-1).reshape(-1, 3).astype(np.float32)
        return (self.origin + (idx * self.spacing).astype(np.float32)).astype(np.float32)

    def bake(self, visibility=False, d=8, dmax=None, reflections=False, levels=None, **kw):
        """probe_sh_device on the grid's points (its keywords: m, spp, max_bounce, seed, jitter, photon_maps, chunk_rays, stream);
        the results stay on the device as .sh [probes,9,3], .hits [probes] and .tmin [probes] -> self.  visibility=True bakes with
        probevis_sh_device and keeps .moments [probes,6,d,d,2] for shade_device(visibility=True); dmax=None becomes 1.5 |spacing|
        (fp32: 1.5 times the cell's diagonal) and is kept as .dmax.  Without it .moments is None.  reflections=True asks the same
        bake for the cubes (m a power of two), prefilters them on the same stream (reflprobe_prefilter_device, `levels` levels, None:
        all) and keeps .chain [probes,T,3], .m and .levels for reflect_device(); the cubes are dropped, level 0 being their copy.
        Without it .chain is None.  The two combine, and neither changes a bit of the other outputs.  Only enqueues."""
        import torch
        pts = torch.from_numpy(self.points()).to(torch.device("cuda", self.ctx.device_id))
        if reflections:
            if kw.get("cube") is not None:
                raise ValueError("cube: bake(reflections=True) asks for the cubes itself")
            lay = reflprobe_layout(kw.get("m", 16), levels)   # (refused before anything is traced)
            kw = dict(kw, cube=True)
        if visibility:
            if dmax is None:
                sp = self.spacing
                dmax = np.float32(1.5) * np.sqrt(((sp[0] * sp[0] + sp[1] * sp[1]).astype(np.float32) + sp[2] * sp[2]).astype(np.float32)).astype(np.float32)
            out = self.ctx.probevis_sh_device(pts, d=d, dmax=float(np.float32(dmax)), **kw)
            self.moments, self.d, self.dmax = out["moments"], int(d), np.float32(dmax)
        else:
            out = self.ctx.probe_sh_device(pts, **kw)
            self.moments = self.d = self.dmax = None
        self.sh, self.hits, self.tmin = out["sh"], out["hits"], out["tmin"]
        if reflections:
            self.chain = self.ctx.reflprobe_prefilter_device(out["cube"], lay["levels"], stream=kw.get("stream"))
            self.m, self.levels = int(kw.get("m", 16)), lay["levels"]
        else:
            self.chain = self.m = self.levels = None
        return self

    def shade_device(self, points, normals, out=None, stream=None, visibility=False, normal_bias=0.0):
        """qa_probe_grid_shade_device: the diffuse light at points (float32 [n,3] CUDA tensor) with unit normals [n,3] from the baked
        grid: the 27 coefficients interpolated trilinearly between the probes of the point's cell (points outside take the
        nearest cell's edge), shaded as Context.probe_shade_device shades -> out float32 [n,3] (given, or allocated).  A point
        or normal that is not finite shades to 0.  visibility=True (qa_probevis_grid_shade_device; the grid was baked with
        visibility=True) weighs each of the cell's eight probes by its trilinear weight, a wrapped cosine towards the probe and
        the Chebyshev bound, from the probe's distance moments, on what it sees at the point's distance - a probe behind a wall
        keeps a floor of 0.05 - and normalises; the point is moved by normal_bias * normal for that test.  Only enqueues."""
        import torch
        if self.sh is None:
            raise ValueError("the grid is not baked: bake() first")
        if visibility and self.moments is None:
            raise ValueError("the grid has no moments: bake(visibility=True) first")
        dev = torch.device("cuda", self.ctx.device_id)
        if not isinstance(points, torch.Tensor):
            raise TypeError(f"points: a torch tensor is expected, not {type(points).__name__}")
        n = _ray_count("points", points)
        _ray_tensor("points", points, (n, 3), torch.float32, dev)
        _ray_tensor("normals", normals, (n, 3), torch.float32, dev)
        out = torch.empty((n, 3), dtype=torch.float32, device=dev) if out is None else out
        _ray_tensor("out", out, (n, 3), torch.float32, dev)
        sptr = Context._stream_arg(stream, points)
        if visibility:
            par = ProbeVisParams.of(self.d, float(self.dmax), normal_bias)
            _check(lib().qa_probevis_grid_shade_device(self.ctx._h, n, self.sh.data_ptr(), self.moments.data_ptr(), self.d, self.origin.ctypes.data,
                                                       self.spacing.ctypes.data, self.counts.ctypes.data, points.data_ptr() or None,
                                                       normals.data_ptr() or None, C.byref(par), out.data_ptr() or None, sptr))
            return out
        _check(lib().qa_probe_grid_shade_device(self.ctx._h, n, self.sh.data_ptr(), self.origin.ctypes.data, self.spacing.ctypes.data, self.counts.ctypes.data,
                                                points.data_ptr() or None, normals.data_ptr() or None, out.data_ptr() or None, sptr))
        return out

    def reflect_device(self, points, dirs, level, out=None, stream=None):
        """qa_reflprobe_grid_shade_device: what a glossy surface at points (float32 [n,3] CUDA tensor) sees along dirs [n,3] (the
        reflected directions, any length) at level [n] (float32; hip.reflprobe_level gives it for a glossiness) from the grid baked
        with reflections=True: Context.reflprobe_shade_device's lookup in each of the eight probes of the point's cell, blended
        trilinearly (points outside take the nearest cell's edge) -> out float32 [n,3] (given, or allocated).  A point on a probe
        takes that probe's answer; a point or direction that is not finite, a zero direction or a NaN level gives 0.  Every probe is
        asked for the same direction (no parallax correction), and a probe behind a wall counts as any other.  Only enqueues."""
        import torch
        if self.chain is None:
            raise ValueError("the grid has no chains: bake(reflections=True) first")
        dev = torch.device("cuda", self.ctx.device_id)
        if not isinstance(points, torch.Tensor):
            raise TypeError(f"points: a torch tensor is expected, not {type(points).__name__}")
        n = _ray_count("points", points)
        _ray_tensor("points", points, (n, 3), torch.float32, dev)
        _ray_tensor("dirs", dirs, (n, 3), torch.float32, dev)
        _ray_tensor("level", level, (n,), torch.float32, dev)
        out = torch.empty((n, 3), dtype=torch.float32, device=dev) if out is None else out
        _ray_tensor("out", out, (n, 3), torch.float32, dev)
        sptr = Context._stream_arg(stream, points)
        _check(lib().qa_reflprobe_grid_shade_device(self.ctx._h, n, self.chain.data_ptr(), self.m, self.levels, self.origin.ctypes.data,
                                                    self.spacing.ctypes.data, self.counts.ctypes.data, points.data_ptr() or None, dirs.data_ptr() or None,
                                                    level.data_ptr() or None, out.data_ptr() or None, sptr))
        return out
