"""QA_RADIANCE_PHOTON_MAPS without a GPU (include/qaray_hip.h; qaray_amd/hip.py; qa_radiance_pm.hip, qa_irradiance_pm.hip): the flag's
value in the header and in Python, the keyword on the five Python calls, the bit RadianceParams sets, and the two new units in the
library's source list."""
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from qaray_amd import hip

HEADER = open(os.path.join(ROOT, "include", "qaray_hip.h")).read()
CALLS = ("radiance_rays_device", "radiance_rays", "irradiance_points_device", "irradiance_points", "bake_light")


def bare_context():
    """A Context object without a context behind it (tests/test_irradiance_host.py): the argument checks come before any library call"""
    c = object.__new__(hip.Context)
    c.device_id, c._h = 0, None
    return c


def test_the_flag_is_bit_3_in_the_header_and_in_python():
    m = re.search(r"^#define\s+QA_RADIANCE_PHOTON_MAPS\s+(\w+)\s*$", HEADER, flags=re.M)
    assert m and m.group(1) == "8u"
    assert hip.QA_RADIANCE_PHOTON_MAPS == 8
    # the bits the existing tests pin as unknown stay free of it
    assert hip.QA_RADIANCE_PHOTON_MAPS & (hip.QA_RADIANCE_PER_SAMPLE | hip.QA_RADIANCE_MISS_ENVIRONMENT | 4) == 0


def test_radiance_params_set_the_bit():
    assert hip.RadianceParams.of(2, 3, 7).flags == 0
    assert hip.RadianceParams.of(2, 3, 7, photon_maps=True).flags == 8
    p = hip.RadianceParams.of(2, 3, 7, per_sample=True, miss_environment=True, photon_maps=True)
    assert (p.spp, p.max_bounce, p.seed, p.flags) == (2, 3, 7, 1 | 2 | 8)


def test_the_five_python_calls_take_photon_maps():
    """radiance_rays(_device) list the keyword; the point calls and bake_light, whose listed defaults tests/test_irradiance_host.py
    pins, take it as their one extra keyword, say so in their docstrings, and refuse any other."""
    c = bare_context()
    for name in CALLS:
        fn = getattr(hip.Context, name)
        sig = inspect.signature(fn)
        listed = "photon_maps" in sig.parameters and sig.parameters["photon_maps"].default is False
        extra = any(p.kind is inspect.Parameter.VAR_KEYWORD for p in sig.parameters.values())
        assert listed or extra, name
        assert "photon_maps" in fn.__doc__, name
    p = np.zeros((5, 3), np.float32)
    # taken: the call goes on to its argument checks (a shape error), which come before the library
    with pytest.raises(ValueError):
        c.irradiance_points(p, p[:4], photon_maps=True)
    with pytest.raises(ValueError):
        c.radiance_rays(p, p[:4], photon_maps=True)
    with pytest.raises(TypeError):
        c.irradiance_points_device(p, p, photon_maps=True)   # numpy where a tensor is expected
    with pytest.raises(TypeError):
        c.radiance_rays_device(p, p, photon_maps=True)
    # any other keyword is refused by name
    for name, args in (("irradiance_points", (p, p)), ("irradiance_points_device", (p, p)), ("bake_light", (3, 0))):
        with pytest.raises(TypeError, match="photon_map"):
            getattr(c, name)(*args, photon_map=True)


def test_the_new_units_are_in_the_source_list():
    text = open(os.path.join(ROOT, "qaray_amd", "csrc", "Makefile")).read()
    m = re.search(r"^HIP_SRCS\s*:=((?:.*\\\n)*.*)$", text, flags=re.M)
    srcs = m.group(1).replace("\\\n", " ").split()
    for unit in ("hip/qa_radiance_pm.hip", "hip/qa_irradiance_pm.hip"):
        assert unit in srcs and os.path.exists(os.path.join(ROOT, "qaray_amd", "csrc", unit)), unit
    kernels = open(os.path.join(ROOT, "qaray_amd", "csrc", "hip", "qa_kernel.h")).read()
    for k in ("qa_integrate_rays_pm", "qa_integrate_points_pm"):
        assert re.search(r"template <bool RES, bool TEX, bool AREA>\s*\n__global__ __launch_bounds__\(QA_BLOCK, QA_WAVES_FOR\(RES, true\)\) void " + k + r"\(", kernels), k
