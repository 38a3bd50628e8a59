"""Cross-stream ordering of a frame that gathers and a flagged batch (QA_RADIANCE_PHOTON_MAPS): both use the context's one heap slab
of the photon gathers, and what keeps them apart is lastFrame, which a batch waits for and records as a frame does (DESIGN.md
"Streams: who waits for whom").  The stall-and-check harness is tests/stream_order_util.py's: one stream is held, so the producer
really is late; the consumer on the other stream must not finish first (event order), and both calls' bits are the serial run's.

The frame is the 47 x 40 REGION at 3 spp with no chunk option; the batch is 256 camera rays, and 256 points."""
import pytest

import stream_order_util as U
from gbuffer_util import REGION
from radiance_photon_util import CUSTOM, case
from test_gpu_stream_order import filled

pytestmark = pytest.mark.gpu

SPP = 3
RAYS = (8, 8, 24, 24)   # 256 camera rays


@pytest.fixture(scope="module")
def streams():
    """Two streams of the caller's that really run side by side (tests/test_gpu_stream_order.py)"""
    import torch
    dev = torch.device("cuda", 0)
    a = torch.cuda.Stream(dev)
    U.calibrate(a)
    b = U.concurrency_control(a, [torch.cuda.Stream(dev) for _ in range(4)])
    yield a, b
    torch.cuda.synchronize()


def setup():
    """A fresh context with custom_photon.xml and its maps, 256 camera rays and the points they hit"""
    import torch
    from qaray_amd import hip
    blob, pm, cm, _ = case(CUSTOM)
    c = hip.Context(0)
    c.upload_scene(blob.copy())
    c.build_photon_maps(pm, cm)
    o, d = c.camera_rays_device(RAYS, seed=3)
    hit = c.cast_rays_device(o, d)
    c.synchronize()
    torch.cuda.synchronize()
    return {"ctx": c, "close": c.close, "o": o, "d": d, "p": hit["point"], "n": hit["normal"]}


def frame(st, s, seed=1):
    import torch
    h, w = REGION[3] - REGION[1], REGION[2] - REGION[0]
    out = {"rgb": filled(s, (h, w, 3), torch.float32), "depth": filled(s, (h, w), torch.float32), "ns": filled(s, (h, w), torch.int32)}
    st["ctx"].render_region_device(REGION, SPP, out["rgb"], out["depth"], out["ns"], seed=seed, stream=s.cuda_stream)
    return out


def rays(st, s):
    import torch
    return st["ctx"].radiance_rays_device(st["o"], st["d"], spp=2, seed=5, miss_environment=True, rgb=filled(s, (256, 3), torch.float32),
                                          t=filled(s, (256,), torch.float32), ns=filled(s, (256,), torch.int32), stream=s.cuda_stream, photon_maps=True)


def points(st, s):
    import torch
    return st["ctx"].irradiance_points_device(st["p"], st["n"], spp=2, seed=5, rgb=filled(s, (256, 3), torch.float32), ns=filled(s, (256,), torch.int32),
                                              stream=s.cuda_stream, photon_maps=True)


def warm(call):
    """The context's first frame (the Halton table, the tile order's upload and its synchronize) and the batch's first launch happen
    here, not behind the hold"""
    def run(st, s):
        frame(st, s, seed=9)
        call(st, s)
    return run


@pytest.mark.parametrize("name,batch", [("rays", rays), ("points", points)])
def test_a_frame_that_gathers_and_a_flagged_batch_wait_for_each_other(streams, name, batch):
    a, b = streams
    U.ordered(f"photon frame->{name}", setup, lambda st, s: frame(st, s, 1), batch, a, b, warm=warm(batch))
    U.ordered(f"photon {name}->frame", setup, batch, lambda st, s: frame(st, s, 2), a, b, warm=warm(batch))
