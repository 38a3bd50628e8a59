"""What the tests of QA_RADIANCE_PHOTON_MAPS share (qa_radiance_pm.hip, qa_irradiance_pm.hip): the scene list - every scene with the
sizes of its maps and the <RES, TEX, AREA> instance of the gathering kernels it runs - and the flagged form of the anchor's batch.
Frames, region and seeds are gbuffer_util's; the frame is radiance_util's.

Map sizes are the existing photon tests' (tests/test_gpu_photon.py, the meta of tests/golden/photon); for
example_project10_objects.xml, which no photon test renders, trc_scene_xmas.xml's.  tests/test_radiance_photon_oracle.py checks on
the CPU that every (scene, sizes) pair fills both maps."""
from conftest import load_photon_golden
from gbuffer_util import REGION, scene_blob
from radiance_util import QA_LIGHT_POINT

CUSTOM = "custom_photon.xml"
CUSTOM_POINT = "custom_photon.xml with point lights"
GLASS = "trc_mtl_glass.xml"
GLASS_AREA = "trc_mtl_glass.xml with an area light"
XMAS = "trc_scene_xmas.xml"
TOWER = "trc_scene_tower.xml"
TOWER_AREA = "trc_scene_tower.xml with an area light"
OBJECTS = "example_project10_objects.xml"
OBJECTS_POINT = "example_project10_objects.xml with point lights"
GOLDENS = ("pm_custom_64x48_2spp", "pm_glass_48x36_2spp", "pm_glossy_shortpaths_48x36_2spp")

# scene -> (photon map, caustics map, (RES, TEX, AREA)); the goldens' sizes come from their meta
SCENES = {
    CUSTOM: ((3000, 20, 0.2), (400, 20, 1.0), (0, 1, 1)),          # (one of its three point lights has a size)
    CUSTOM_POINT: ((3000, 20, 0.2), (400, 20, 1.0), (0, 1, 0)),
    GOLDENS[0]: (None, None, (0, 1, 1)),
    GOLDENS[1]: (None, None, (1, 0, 0)),
    GOLDENS[2]: (None, None, (1, 0, 0)),
    GLASS: ((3000, 20, 1.5), (400, 20, 2.5), (1, 0, 0)),
    GLASS_AREA: ((3000, 20, 1.5), (400, 20, 2.5), (1, 0, 1)),
    XMAS: ((3000, 20, 0.5), (300, 20, 1.0), (0, 0, 0)),
    TOWER: ((2000, 20, 1.0), (100, 20, 2.0), (0, 0, 0)),
    TOWER_AREA: ((2000, 20, 1.0), (100, 20, 2.0), (0, 0, 1)),
    OBJECTS: ((3000, 20, 0.5), (300, 20, 1.0), (1, 1, 1)),
    OBJECTS_POINT: ((3000, 20, 0.5), (300, 20, 1.0), (1, 1, 0)),
}
INSTANCES = {(res, tex, area) for res in (0, 1) for tex in (0, 1) for area in (0, 1)}   # every one is compiled


def case(scene):
    """-> (blob at gbuffer_util.SIZE, photon map sizes, caustics map sizes, (RES, TEX, AREA))"""
    from qaray_amd import hip
    pm, cm, inst = SCENES[scene]
    if scene in GOLDENS:
        meta = load_photon_golden(scene)["meta"]
        return scene_blob(meta["scene"]), tuple(meta["photon"]), tuple(meta["caustics"]), inst
    name = scene.split(" with ")[0]
    blob = scene_blob(name)
    if scene != name:
        blob = blob.copy()
        lights = hip.blob_table(blob, "lights")
        if scene.endswith("point lights"):
            assert (lights["size"] > 0.01).any()
            lights["size"] = 0   # (tests/test_gpu_irradiance.py POINT_LIT_OBJECTS)
        else:
            point = lights["type"] == QA_LIGHT_POINT
            assert point.sum() == 1 and not (lights["size"] > 0.01).any()
            lights["size"][point] = 1.5   # (radiance_util.AREA_BOX)
    return blob, pm, cm, inst


def instance(kernel_name):
    """(RES, TEX, AREA) of the kernel_name() of a frame with maps built, which must say PHOTON=1"""
    assert "PHOTON=1" in kernel_name and "LIGHTS=1" in kernel_name, kernel_name
    return tuple(int(f"{k}=1" in kernel_name) for k in ("RES", "TEX", "AREA"))


def flagged_batch_of_own_rays(c, spp, seed, max_bounce=5, photon_maps=True):
    """radiance_util.batch_of_own_rays with the flag: radiance_rays_device(camera_sample_rays_device(REGION, 0, spp, all outputs),
    per sample, photon_maps) -> (rgb, t, ns) numpy, the counters of that batch alone, and the rays (tensors)"""
    rays = c.camera_sample_rays_device(REGION, 0, spp)
    c.reset_counters()
    out = c.radiance_rays_device(rays["origins"], rays["dirs"], spp=spp, max_bounce=max_bounce, seed=seed, dx=rays["dx"], dy=rays["dy"],
                                 screen=rays["screen"], stream_ids=rays["stream_ids"], photon_maps=photon_maps)
    c.synchronize()
    return tuple(a.cpu().numpy() for a in out), c.counters(), rays
