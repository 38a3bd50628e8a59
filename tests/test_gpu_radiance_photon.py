"""Radiance queries that gather from built photon maps (QA_RADIANCE_PHOTON_MAPS; qa_radiance_pm.hip, whose opening comment is the
specification).  The anchor is tests/test_gpu_radiance.py's with maps: the renderer's own camera rays of every sample, handed back
in with the flag, reproduce the frame that gathers bit for bit - which ties the flagged call to the reference's goldens and to the
CPU oracle through tests/test_gpu_photon.py.  The rest checks independence of batch and lane (the heap slab's slots are reused by
persistent waves), determinism and scratch, state and refusals.  Every comparison is bit for bit.

Frames stay at spp <= 3 on the 47 x 40 REGION, and no chunk option is set."""
import numpy as np
import pytest

from gbuffer_util import MISS, REGION, SEEDS, bits
from radiance_photon_util import CUSTOM, GLASS, GLASS_AREA, INSTANCES, SCENES, case, flagged_batch_of_own_rays, instance
from radiance_util import N, QA_ENOSCENE, QA_EUNSUPPORTED, frame
from ray_query_util import fresh

pytestmark = pytest.mark.gpu

DIFFER = (CUSTOM, GLASS)   # where the flagged batch must differ from the batch without maps (the goldens' scenes: their frames do)
_RAN = {}                  # scene -> (RES, TEX, AREA) as the anchor met it


def with_maps(scene):
    blob, pm, cm, inst = case(scene)
    c = fresh(blob)
    c.build_photon_maps(pm, cm)
    return c, blob, inst


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


@pytest.mark.parametrize("scene", list(SCENES))
def test_own_camera_rays_handed_back_in_with_the_flag_are_the_frame_that_gathers(scene):
    """Check 1: with maps built, radiance_rays_device(camera_sample_rays_device(region, 0, spp), per sample, photon_maps=True) is
    render_region_device's rgb, depth and ns bit for bit at spp 1 and 3, and moves the counters as the frame does.  The frame's
    kernel_name() names the instance (the gathering batch kernels are picked by the same predicates)."""
    c, _, inst = with_maps(scene)
    try:
        for spp, seed in ((1, SEEDS[0]), (3, SEEDS[1])):
            (f_rgb, f_depth, f_ns), f_cnt = frame(c, spp, seed)
            name = c.kernel_name()
            assert instance(name) == inst, (scene, name)
            _RAN[scene] = instance(name)
            (rgb, t, ns), cnt, _ = flagged_batch_of_own_rays(c, spp, seed)
            assert c.kernel_name() == name   # (what the last frame ran on: a batch leaves it alone)
            assert np.array_equal(ns, f_ns) and (ns == spp).all(), (scene, spp)
            assert np.array_equal(bits(t), bits(f_depth)), (scene, spp)
            assert np.array_equal(bits(rgb), bits(f_rgb)), (scene, spp, int((bits(rgb) != bits(f_rgb)).any(axis=1).sum()))
            for k in ("samples", "casts_normal", "casts_shadow"):
                assert cnt[k] == f_cnt[k], (scene, spp, k)
            assert cnt["samples"] == N * spp
        # the maps arrive: the same batch without them differs somewhere (same first hits: the gathers draw nothing)
        c.clear_photon_maps()
        (p_rgb, p_t, p_ns), _, _ = flagged_batch_of_own_rays(c, spp, seed, photon_maps=False)
        differ = int((bits(p_rgb) != bits(rgb)).any(axis=1).sum())
        print(scene, "rays whose radiance the maps change:", differ, "of", N)
        assert np.array_equal(bits(p_t), bits(t)) and np.array_equal(p_ns, ns)
        if scene in DIFFER:
            assert differ > 0, scene
    finally:
        c.close()


def test_the_anchor_reaches_all_eight_instances():
    """Every compiled instance of qa_integrate_rays_pm<RES, TEX, AREA> is run by a scene of check 1, which asserts the instance it ran."""
    assert {inst for _, _, inst in SCENES.values()} == INSTANCES
    assert all(_RAN[s] == SCENES[s][2] for s in _RAN)


def test_a_rays_answer_does_not_depend_on_its_batch_or_its_lane():
    """Check 2, on custom_photon.xml: batches of 1, 63, 64, 65 and 130 rays with stream ids, and a permutation, equal the largest
    batch's rows; one batch of multi_processor_count * 8 * 256 + 65 rays - more work items than the capped grid has waves, so
    persistent waves reuse heap slots - made of the 130 rays repeated with their stream ids: its first and last 130 rows equal the
    small batch's."""
    import torch
    rng = np.random.default_rng(20261021)
    c, _, _ = with_maps(CUSTOM)
    try:
        o, d = c.camera_rays(REGION, SEEDS[0])
        pick = rng.choice(len(o), 130, replace=False)
        o, d = o[pick], d[pick]
        ids = rng.integers(0, 1 << 20, 130).astype(np.uint32)
        kw = dict(spp=2, max_bounce=3, seed=SEEDS[1], miss_environment=True, photon_maps=True)
        whole = c.radiance_rays(o, d, stream_ids=ids, **kw)
        assert (whole[2] == 2).all() and (whole[1] != MISS).sum() > 60 and len(np.unique(whole[0], axis=0)) > 60
        for n in (1, 63, 64, 65, 130):
            part = c.radiance_rays(o[:n], d[:n], stream_ids=ids[:n], **kw)
            perm = rng.permutation(n)
            shuffled = c.radiance_rays(o[:n][perm], d[:n][perm], stream_ids=ids[:n][perm], **kw)
            for a, b, w in zip(part, shuffled, whole):
                assert np.array_equal(bits(a), bits(w[:n])), n
                assert np.array_equal(bits(b), bits(w[:n][perm])), n
        big = torch.cuda.get_device_properties(0).multi_processor_count * 8 * 256 + 65
        row = torch.arange(big, device="cuda:0") % 130
        out = c.radiance_rays_device(dev(o)[row].contiguous(), dev(d)[row].contiguous(), stream_ids=dev(ids.view(np.int32))[row].contiguous(), **kw)
        c.synchronize()
        row = row.cpu().numpy()
        for a, w in zip(out, whole):
            a = a.cpu().numpy()
            assert np.array_equal(bits(a[:130]), bits(w[row[:130]])) and np.array_equal(bits(a[-130:]), bits(w[row[-130:]]))
            assert np.array_equal(bits(a), bits(w[row])), "every repetition is the ray"
    finally:
        c.close()


@pytest.mark.parametrize("scene", [CUSTOM, GLASS])
def test_the_same_call_gives_the_same_bits_whatever_the_scratch_holds(scene):
    """Check 3: the same flagged batch three times, then after scrub_scratch(0) and scrub_scratch(0xFFFFFFFF): the same bits (a
    spill store ahead of the exec restore, DESIGN 5b, shows exactly there)."""
    c, _, _ = with_maps(scene)
    try:
        first, _, _ = flagged_batch_of_own_rays(c, 3, SEEDS[1])
        for pattern in (None, None, 0, 0xFFFFFFFF):
            if pattern is not None:
                c.scrub_scratch(pattern)
            again, _, _ = flagged_batch_of_own_rays(c, 3, SEEDS[1])
            for a, b in zip(again, first):
                assert np.array_equal(bits(a), bits(b)), (scene, pattern)
        assert (first[0] > 0).any()
    finally:
        c.close()


def test_state_and_refusals():
    """Check 4: the flag without maps is QA_ENOSCENE and writes nothing - before a build, after clear_photon_maps(), after
    edit_materials (which drops the maps); without the flag a context with maps still refuses (QA_EUNSUPPORTED); after edit_camera
    the maps survive and the flagged batch is the frame of the new camera; the numpy forms agree with the device forms."""
    import torch
    from qaray_amd import hip
    blob, pm, cm, _ = case(CUSTOM)
    c = fresh(blob)
    try:
        o, d = (x[::5] for x in c.camera_rays(REGION, SEEDS[0]))
        n = len(o)
        to, td = dev(o), dev(d)
        rgb = torch.full((n, 3), 7.0, device="cuda:0")
        tt = torch.full((n,), 7.0, device="cuda:0")
        ns = torch.full((n,), 7, dtype=torch.int32, device="cuda:0")
        kw = dict(spp=2, seed=SEEDS[1], miss_environment=True)

        def refused(code):
            with pytest.raises(hip.HipError) as e:
                c.radiance_rays_device(to, td, rgb=rgb, t=tt, ns=ns, photon_maps=True, **kw)
            assert e.value.code == code and (code != QA_ENOSCENE or "no photon maps built" in str(e.value))
            with pytest.raises(hip.HipError) as e:
                c.radiance_rays(o, d, photon_maps=True, **kw)
            assert e.value.code == code
            c.synchronize()
            assert (rgb == 7.0).all() and (tt == 7.0).all() and (ns == 7).all()   # a refusal writes nothing

        refused(QA_ENOSCENE)                       # no maps yet
        c.build_photon_maps(pm, cm)
        with pytest.raises(hip.HipError) as e:     # maps, no flag: today's refusal
            c.radiance_rays_device(to, td, rgb=rgb, t=tt, ns=ns, **kw)
        assert e.value.code == QA_EUNSUPPORTED
        got = c.radiance_rays_device(to, td, photon_maps=True, **kw)
        c.synchronize()
        host = c.radiance_rays(o, d, photon_maps=True, **kw)
        for a, b in zip(got, host):
            assert np.array_equal(bits(a.cpu().numpy()), bits(b))
        assert (host[2] == 2).all() and (host[0] > 0).any()
        c.clear_photon_maps()
        refused(QA_ENOSCENE)
        c.build_photon_maps(pm, cm)
        mats = hip.blob_table(blob, "materials")
        c.edit_materials(0, mats[:1])              # (the same record: every material edit drops the maps)
        refused(QA_ENOSCENE)
        # a camera edit keeps the maps: the flagged batch of the new camera's rays is the new camera's frame
        c.build_photon_maps(pm, cm)
        cam = hip.blob_camera(blob).copy()
        cam["cam_pos"] = cam["cam_pos"] + np.float32([0.5, -0.25, 0.75])   # (the image plane stays: another pinhole behind it)
        c.edit_camera(cam)
        assert c.photon_maps_info()[0][0] > 0
        (f_rgb, f_depth, f_ns), f_cnt = frame(c, 2, SEEDS[0])
        (b_rgb, b_t, b_ns), cnt, _ = flagged_batch_of_own_rays(c, 2, SEEDS[0])
        assert np.array_equal(bits(b_rgb), bits(f_rgb)) and np.array_equal(bits(b_t), bits(f_depth)) and np.array_equal(b_ns, f_ns)
        assert all(cnt[k] == f_cnt[k] for k in ("samples", "casts_normal", "casts_shadow"))
    finally:
        c.close()
    # area lights with max_bounce = 8: refused as a frame refuses them, flag or not
    c, _, inst = with_maps(GLASS_AREA)
    try:
        assert inst[2] == 1
        o, d = (x[::5] for x in c.camera_rays(REGION, SEEDS[0]))
        with pytest.raises(hip.HipError) as e:
            c.radiance_rays(o, d, max_bounce=8, photon_maps=True)
        assert e.value.code == QA_EUNSUPPORTED
        assert (c.radiance_rays(o, d, max_bounce=7, photon_maps=True)[2] == 1).all()
    finally:
        c.close()
