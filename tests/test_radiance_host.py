"""The radiance queries' host side without a GPU (qa_radiance.hip; include/qaray_hip.h): the documented defaults through
hip.RadianceParams, the flag values against the header, and the argument checks Python makes before it enters the library."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from qaray_amd import hip

HEADER = open(os.path.join(ROOT, "include", "qaray_hip.h")).read()


def header_define(name):
    return int(re.search(r"#define\s+" + name + r"\s+(\d+)u", HEADER).group(1))


def test_params_default_fills_the_documented_defaults():
    p = hip.RadianceParams.default()
    assert (p.spp, p.max_bounce, p.seed, p.flags) == (1, 5, 0x51A7A7, 0)
    assert p.seed == hip.DEFAULT_SEED   # a batch and a frame called with defaults share their streams
    assert "spp 1, max_bounce 5, seed 0x51A7A7, flags 0" in HEADER
    assert hip.lib().qa_radiance_params_default(None) == -1   # QA_EINVAL, no context needed


def test_flag_values_equal_the_headers():
    assert hip.QA_RADIANCE_PER_SAMPLE == header_define("QA_RADIANCE_PER_SAMPLE") == 1
    assert hip.QA_RADIANCE_MISS_ENVIRONMENT == header_define("QA_RADIANCE_MISS_ENVIRONMENT") == 2
    p = hip.RadianceParams.of(spp=3, max_bounce=2, seed=9, per_sample=True, miss_environment=True)
    assert (p.spp, p.max_bounce, p.seed, p.flags) == (3, 2, 9, 3)
    assert hip.RadianceParams.of(per_sample=True).flags == 1 and hip.RadianceParams.of(miss_environment=True).flags == 2


def test_params_struct_is_the_headers():
    m = re.search(r"typedef struct qa_radiance_params \{([^}]*)\}", HEADER)
    fields = [f.strip() for part in m.group(1).split(";") if part.strip() for f in part.replace("int ", "").replace("uint32_t ", "").split(",")]
    assert fields == [name for name, _ in hip.RadianceParams._fields_]
    import ctypes as C
    assert C.sizeof(hip.RadianceParams) == 16


def test_shapes_are_sorted_out_before_the_library():
    assert hip._radiance_shape("origins", np.zeros((7, 3), np.float32), 4) == (7, False)
    assert hip._radiance_shape("origins", np.zeros((7, 4, 3), np.float32), 4) == (7, True)
    assert hip._radiance_shape("origins", np.zeros((7, 1, 3), np.float32), 1) == (7, True)
    for bad in ((7,), (7, 2), (7, 3, 3), (7, 4, 2), (2, 7, 4, 3)):
        with pytest.raises(ValueError):
            hip._radiance_shape("origins", np.zeros(bad, np.float32), 4)
