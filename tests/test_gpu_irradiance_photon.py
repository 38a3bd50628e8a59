"""Irradiance queries that gather from built photon maps (QA_RADIANCE_PHOTON_MAPS; qa_irradiance_pm.hip, whose opening comment
specifies the gather at the point).  The anchor is tests/test_gpu_irradiance.py's with maps: on a surface whose material is the white
diffuse record, the flagged light at the points cast_rays reports is bit for bit the flagged radiance of the rays that hit them -
which ties the point's own gather to section D's, and through tests/test_gpu_radiance_photon.py to the frame that gathers.  Then: a
caustic arrives at floor points under a glass ball, and void points stay black.  Every comparison is bit for bit.

Radiance and point calls only: no frame is rendered here."""
import numpy as np
import pytest

from gbuffer_util import REGION, SEEDS, bits
from radiance_photon_util import CUSTOM, CUSTOM_POINT, GLASS, GLASS_AREA, GOLDENS, INSTANCES, OBJECTS, OBJECTS_POINT, TOWER_AREA, XMAS, case
from radiance_util import QA_ENOSCENE, QA_EUNSUPPORTED, variant
from ray_query_util import fresh, void_rays
from test_gpu_irradiance import COLOURS, dev, first_hits, white

pytestmark = pytest.mark.gpu

# one scene per instance of qa_integrate_points_pm<RES, TEX, AREA> (radiance_photon_util.SCENES names each scene's)
ANCHOR = (XMAS, TOWER_AREA, CUSTOM_POINT, CUSTOM, GLASS, GLASS_AREA, OBJECTS_POINT, OBJECTS)


def test_the_anchor_reaches_all_eight_instances():
    assert {case(s)[3] for s in ANCHOR} == INSTANCES and len(ANCHOR) == 8


@pytest.mark.parametrize("scene", ANCHOR)
def test_the_flagged_light_at_a_white_surface_is_the_flagged_radiance_of_the_rays_that_hit_it(scene):
    """Check 5.  Among the materials without texmaps that the region's camera rays hit on front faces, the one hit most (150 rays at
    least) is set to the white record; the maps are built after that edit, which drops them.  For the rays that hit it,
    irradiance_points_device(point, normal, photon_maps=True) equals radiance_rays_device(rays, miss_environment, photon_maps=True)
    in rgb and ns, with the pixel's stream id, at spp 1 and 3 and max_bounce 0 and 5.  The scene runs the instance the table names."""
    from qaray_amd import hip
    blob, pm, cm, inst = case(scene)
    c = fresh(blob)
    try:
        o, d, cast = first_hits(c)
        mats = hip.blob_table(blob, "materials")
        word = cast["ids"][:, 1]
        front = (cast["ids"][:, 0] >= 0) & (word >= 0) & (word < hip.QA_GBUFFER_BACKFACE)
        plain = np.array([all(int(m[f]["texmap"]) < 0 for f in COLOURS) for m in mats])
        count = np.bincount(word[front], minlength=len(mats)) * plain
        m = int(count.argmax())
        assert count[m] >= 150, (scene, count)
        c.edit_materials(m, white(mats[m:m + 1]))
        c.build_photon_maps(pm, cm)
        ran = variant(c.kernel_name())   # (RES, LIGHTS, TEX, AREA) of the plan: the gathering kernels are picked by its predicates
        assert ran[1] == 1 and (ran[0], ran[2], ran[3]) == inst, (scene, c.kernel_name())
        sel = front & (word == m)
        sid = dev(np.flatnonzero(sel).astype(np.int32))
        to, td, tp, tn = dev(o[sel]), dev(d[sel]), dev(cast["point"][sel]), dev(cast["normal"][sel])
        lit = False
        for spp, seed in ((1, SEEDS[0]), (3, SEEDS[1])):
            for max_bounce in (0, 5):
                want = c.radiance_rays_device(to, td, spp, max_bounce, seed, stream_ids=sid, miss_environment=True, photon_maps=True)
                got = c.irradiance_points_device(tp, tn, spp, max_bounce, seed, stream_ids=sid, photon_maps=True)
                c.synchronize()
                rgb, ns = got[0].cpu().numpy(), got[1].cpu().numpy()
                w_rgb, w_ns = want[0].cpu().numpy(), want[2].cpu().numpy()
                assert np.array_equal(ns, w_ns) and (ns == spp).all(), (scene, spp, max_bounce)
                differ = (bits(rgb) != bits(w_rgb)).any(axis=1)
                assert not differ.any(), (scene, spp, max_bounce, int(differ.sum()), int(sel.sum()))
                lit = lit or bool((rgb > 0).any())
        assert lit, "some light arrives somewhere"
        # the maps arrive at the points: with them cleared the last call's answer is another somewhere
        c.clear_photon_maps()
        plain_rgb = c.irradiance_points_device(tp, tn, spp, max_bounce, seed, stream_ids=sid)[0]
        c.synchronize()
        print(scene, "points whose light the maps change:", int((bits(plain_rgb.cpu().numpy()) != bits(rgb)).any(axis=1).sum()), "of", int(sel.sum()))
    finally:
        c.close()


def test_a_caustic_arrives_at_the_floor_under_the_glass_ball():
    """Check 6, on the glass golden's scene with its maps: at the floor points the region's camera rays meet, the flagged light
    differs from the light with the maps cleared at some of them - at max_bounce 0 too, where nothing but the point's own gather
    from the caustics map can differ; the 19 void points among them are black and counted; the host form agrees; without maps the
    flag is refused, and with maps the call without it."""
    import torch
    from qaray_amd import hip
    blob, pm, cm, inst = case(GOLDENS[1])
    c = fresh(blob)
    try:
        o, d, cast = first_hits(c)
        word = cast["ids"][:, 1]
        front = (cast["ids"][:, 0] >= 0) & (word >= 0) & (word < hip.QA_GBUFFER_BACKFACE)
        floor = int(np.bincount(word[front]).argmax())
        sel = front & (word == floor)
        gp, gn = cast["point"][sel], cast["normal"][sel]
        assert len(gp) > 500
        vp, vn = void_rays()
        at = np.linspace(0, len(gp), len(vp), dtype=int)
        p, nr = np.insert(gp, at, vp, axis=0), np.insert(gn, at, vn, axis=0)
        void = ~(np.isfinite(p).all(axis=1) & np.isfinite(nr).all(axis=1)) | (nr == 0).all(axis=1)
        assert void.sum() == 19
        ids = np.arange(len(p), dtype=np.uint32)
        tp, tn = dev(p), dev(nr)
        out = torch.full((len(p), 3), 7.0, device="cuda:0")
        with pytest.raises(hip.HipError) as e:
            c.irradiance_points_device(tp, tn, rgb=out, photon_maps=True)
        assert e.value.code == QA_ENOSCENE and "no photon maps built" in str(e.value)
        plain = {b: c.irradiance_points(p, nr, spp=3, max_bounce=b, seed=SEEDS[1], stream_ids=ids) for b in (0, 5)}
        c.build_photon_maps(pm, cm)
        ran = variant(c.kernel_name())
        assert (ran[0], ran[2], ran[3]) == inst
        with pytest.raises(hip.HipError) as e:
            c.irradiance_points_device(tp, tn, rgb=out)
        assert e.value.code == QA_EUNSUPPORTED
        c.synchronize()
        assert (out == 7.0).all()   # a refusal writes nothing
        for b in (0, 5):
            c.reset_counters()
            rgb, ns = c.irradiance_points(p, nr, spp=3, max_bounce=b, seed=SEEDS[1], stream_ids=ids, photon_maps=True)
            assert c.counters()["samples"] == 3 * len(p)
            assert (ns == 3).all() and not bits(rgb[void]).any() and np.isfinite(rgb).all()
            differ = (bits(rgb) != bits(plain[b][0])).any(axis=1)
            print("max_bounce", b, "floor points whose light the maps change:", int(differ.sum()), "of", int((~void).sum()))
            assert differ.any() and not differ[void].any()
            if b == 0:
                assert (rgb[differ] > plain[b][0][differ]).any(), "the point's own gather adds light"
            got = c.irradiance_points_device(tp, tn, 3, b, SEEDS[1], stream_ids=dev(ids.view(np.int32)), photon_maps=True)
            c.synchronize()
            assert np.array_equal(bits(got[0].cpu().numpy()), bits(rgb)) and np.array_equal(got[1].cpu().numpy(), ns)
    finally:
        c.close()
