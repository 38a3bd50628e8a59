"""The variance form of the filter on the device (qa_denoise_variance_device: the pass-0 kernel qa_denoise_pass0<true> of
qa_denoise.hip ahead of the iterate kernels as they are): the device build of the VARIANCE FORM of qa_denoise_dev.h equals the host
build (qa_test_denoise_variance_host, pinned to a restatement of the specification by tests/test_denoise_variance_host.py) bit for
bit; and the claim about quality on the renderer's own frames, accumulated by hip.TemporalPreview(moments=True)."""
import numpy as np
import pytest

import denoise_variance_util as vu
from denoise_variance_util import bits, variance_frame

pytestmark = pytest.mark.gpu

QA_EINVAL = -1


@pytest.fixture(scope="module")
def ctx():
    from qaray_amd import hip
    c = hip.Context(0)
    yield c
    c.close()


def upload(rgb, depth, ns, normal, albedo, var):
    import torch
    dev = torch.device("cuda", 0)
    f = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)   # noqa: E731
    return f(rgb), f(depth), torch.from_numpy(np.ascontiguousarray(ns, np.uint32).view(np.int32)).to(dev), f(normal), f(albedo), f(var)


def device_variance(ctx, frame, stream=None, alias=False, **kw):
    import torch
    t = upload(*frame)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    out = ctx.denoise_variance_device(*t, out=t[0] if alias else None, stream=stream.cuda_stream if stream is not None else None, **kw)
    if stream is not None:
        stream.synchronize()
    else:
        ctx.synchronize()
    for k, (dev, host) in enumerate(zip(t, frame)):   # the inputs are not written
        if dev is not None and not (alias and k == 0):
            assert np.array_equal(dev.cpu().numpy().view(np.uint32), np.ascontiguousarray(host).view(np.uint32)), k
    return out.cpu().numpy()


@pytest.mark.parametrize("w,h", vu.VARIANCE_SIZES)
def test_device_equals_host_bit_for_bit(ctx, w, h):
    """iterations 1, 3 and 5: without guides the LDS kernels at steps 1 and 2 and the direct kernel at steps 4, 8 and 16, with guides
    the guided iterate kernel, each fed by the new pass 0."""
    import torch
    from qaray_amd import hip
    rgb, depth, ns, normal, albedo, var = variance_frame(w, h, 100 * w + h)
    side = torch.cuda.Stream()
    for guides in ((None, None), (normal, albedo), (None, albedo)):
        for iterations, scale in ((1, 4.0), (3, 0.5), (5, 4.0), (0, 4.0)):
            want = bits(hip.denoise_variance_host(rgb, depth, ns, *guides, var, iterations=iterations, variance_scale=scale))
            for stream, alias in ((None, False), (side, True)):
                got = bits(device_variance(ctx, (rgb, depth, ns) + guides + (var,), stream, alias, iterations=iterations, variance_scale=scale))
                bad = np.argwhere(got != want)
                assert bad.size == 0, (guides[0] is not None, guides[1] is not None, iterations, stream is not None, alias, len(bad), bad[:5])
    if w * h > 100:   # (the plane reached the kernels)
        assert not np.array_equal(bits(hip.denoise_variance_host(rgb, depth, ns, None, None, var)), bits(hip.denoise_host(rgb, depth, ns)))


def test_flag_off_is_the_guided_call(ctx):
    rgb, depth, ns, normal, albedo, var = variance_frame(33, 35, 9)
    none = np.full_like(var, -1)
    for guides in ((normal, albedo), (None, None)):
        t = upload(rgb, depth, ns, *guides, None)
        want = ctx.denoise_guided_device(*t[:5])
        ctx.synchronize()
        want = bits(want.cpu().numpy())
        assert np.array_equal(bits(device_variance(ctx, (rgb, depth, ns) + guides + (None,), variance_scale=9.0)), want)
        assert np.array_equal(bits(device_variance(ctx, (rgb, depth, ns) + guides + (none,), variance_scale=9.0)), want)


def test_a_smaller_frame_after_a_larger_one():
    from qaray_amd import hip
    c = hip.Context(0)   # (its own context: the working planes start at the first frame's size)
    try:
        small, large = variance_frame(16, 16, 1), variance_frame(67, 45, 2)
        first = device_variance(c, small)
        assert np.array_equal(bits(device_variance(c, large)), bits(hip.denoise_variance_host(*large)))
        assert np.array_equal(bits(device_variance(c, small[:3] + (None, None) + small[5:])), bits(hip.denoise_variance_host(*small[:3], None, None, small[5])))
        assert np.array_equal(bits(device_variance(c, small)), bits(first))
        assert np.array_equal(bits(first), bits(hip.denoise_variance_host(*small)))
    finally:
        c.close()


def test_the_variance_plane_helps_on_the_renderers_accumulated_previews(ctx):
    """Section 4 of DESIGN.md 4k on device frames: eight 4-spp frames through hip.TemporalPreview(moments=True), the accumulated frame
    filtered by denoise_guided_device (i) and by denoise_variance_device with tp.variance (ii), defaults, both guides of
    gbuffer_device; luma RMSE to 256 spp.  Measured on one MI355X, raw / accumulated / (i) / (ii): custom_textures.xml 0.0324 / 0.0276 /
    0.0300 / 0.0264, (ii) / (i) = 0.880; Cornell box 0.8860 / 0.5476 / 0.5157 / 0.4953, (ii) / (i) = 0.961; every pixel trusted."""
    t, b = vu.device_quality(ctx, "textures"), vu.device_quality(ctx, "box")
    for name, q in (("custom_textures.xml", t), ("Cornell box", b)):
        print(f"{name}: raw {q['raw']:.4f}, accumulated {q['acc']:.4f}, guided (i) {q['i']:.4f}, variance form (ii) {q['ii']:.4f}, "
              f"(ii) / (i) {q['ii'] / q['i']:.4f}, trusted {q['trusted']:.3f}")
    assert t["trusted"] > 0.9 and b["trusted"] > 0.9
    assert t["ii"] < t["i"]
    assert b["ii"] <= 1.02 * b["i"]
    assert t["ii"] < t["raw"] and b["ii"] < b["raw"]


def test_invalid_arguments_are_refused(ctx):
    import ctypes as C
    from qaray_amd import hip
    frame = variance_frame(7, 5, 3)
    t = upload(*frame)
    for kw in ({"iterations": 7}, {"variance_scale": 0.0}, {"variance_scale": float("nan")}, {"sigma_normal": 0.0}):
        with pytest.raises(hip.HipError) as e:
            ctx.denoise_variance_device(*t, **kw)
        assert e.value.code == QA_EINVAL, kw
    L, ok = hip.lib(), hip.DenoiseVarianceParams.default()
    ptr = [x.data_ptr() for x in t]
    assert L.qa_denoise_variance_device(ctx._h, ptr[0], ptr[1], ptr[2], ptr[3], ptr[4], None, 7, 5, C.byref(ok), ptr[0], None) == QA_EINVAL   # bit without plane
    ok.flags = 3
    assert L.qa_denoise_variance_device(ctx._h, ptr[0], ptr[1], ptr[2], ptr[3], ptr[4], ptr[5], 7, 5, C.byref(ok), ptr[0], None) == QA_EINVAL   # plane without bit
    ok.flags = 8
    assert L.qa_denoise_variance_device(ctx._h, ptr[0], ptr[1], ptr[2], None, None, None, 7, 5, C.byref(ok), ptr[0], None) == QA_EINVAL
    ok.flags = 7
    assert L.qa_denoise_variance_device(ctx._h, None, ptr[1], ptr[2], ptr[3], ptr[4], ptr[5], 7, 5, C.byref(ok), ptr[0], None) == QA_EINVAL
    assert L.qa_denoise_variance_device(ctx._h, ptr[0], ptr[1], ptr[2], ptr[3], ptr[4], ptr[5], 7, 5, None, ptr[0], None) == QA_EINVAL
    assert L.qa_denoise_variance_device(ctx._h, ptr[0], ptr[1], ptr[2], ptr[3], ptr[4], ptr[5], 7, 5, C.byref(ok), ptr[0], None) == 0
    ctx.synchronize()
