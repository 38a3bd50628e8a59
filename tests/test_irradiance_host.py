"""The irradiance queries' host side without a GPU (qa_irradiance.hip; include/qaray_hip.h): the documented defaults of the Python
calls, the entries the library exports against the header, and the argument checks Python makes before it enters the library."""
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from qaray_amd import hip

HEADER = open(os.path.join(ROOT, "include", "qaray_hip.h")).read()


def defaults(fn):
    return {k: p.default for k, p in inspect.signature(fn).parameters.items() if p.default is not inspect.Parameter.empty}


def bare_context():
    """A Context object without a context behind it: what the argument checks run on (they come before any library call)"""
    c = object.__new__(hip.Context)
    c.device_id, c._h = 0, None
    return c


def test_parameter_defaults():
    assert defaults(hip.Context.irradiance_points_device) == dict(spp=16, max_bounce=5, seed=hip.DEFAULT_SEED, stream_ids=None, rgb=None, ns=None, stream=None)
    assert defaults(hip.Context.irradiance_points) == dict(spp=16, max_bounce=5, seed=hip.DEFAULT_SEED, stream_ids=None)
    assert defaults(hip.Context.bake_light) == dict(spp=64, max_bounce=5, scale=1.0, mtl=-1, dilate=2, seed=hip.DEFAULT_SEED, stream=None)
    assert list(inspect.signature(hip.Context.bake_light).parameters)[:3] == ["self", "node", "texmap"]
    # the parameters are a qa_radiance_params without flags: the library's own defaults behind the ones given
    p = hip.RadianceParams.of(16, 5, hip.DEFAULT_SEED)
    assert (p.spp, p.max_bounce, p.seed, p.flags) == (16, 5, 0x51A7A7, 0)
    assert "paths that return to the node read" in hip.Context.bake_light.__doc__


def test_the_entries_are_exported_as_the_header_declares_them():
    L = hip.lib()
    text = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    found = {m.group(1): [a.strip() for a in m.group(2).split(",")] for m in re.finditer(r"\bint\s+(qa_irradiance\w*)\s*\(([^;{}()]*)\)\s*;", text)}
    assert sorted(found) == ["qa_irradiance_points", "qa_irradiance_points_device"]
    for name, args in found.items():
        fn = getattr(L, name)   # (AttributeError: the symbol is not exported)
        assert len(fn.argtypes) == len(args), name
        assert any(a.startswith("const qa_radiance_params *") for a in args), name
    assert found["qa_irradiance_points_device"][-1] == "void *stream"
    assert found["qa_irradiance_points_device"][:-1] == [a.replace("points", "d_points").replace("normals", "d_normals").replace("stream_ids", "d_stream")
                                                         .replace("*rgb", "*d_rgb").replace("*nsamples", "*d_nsamples") for a in found["qa_irradiance_points"]]
    # without a context both refuse before anything else
    assert L.qa_irradiance_points_device(None, 1, None, None, None, None, None, None, None) == -1
    assert L.qa_irradiance_points(None, 1, None, None, None, None, None, None) == -1


def test_argument_checks_come_before_the_library():
    import torch
    c = bare_context()
    p = np.zeros((5, 3), np.float32)
    with pytest.raises(TypeError):
        c.irradiance_points_device(p, p)                                   # numpy where a tensor is expected
    with pytest.raises(ValueError):
        c.irradiance_points_device(torch.zeros((5, 3)), torch.zeros((5, 3)))   # a CPU tensor
    with pytest.raises(ValueError):
        c.irradiance_points_device(torch.zeros((5, 4)), torch.zeros((5, 4)))   # shape
    with pytest.raises(ValueError):
        c.irradiance_points(p, p[:4])
    with pytest.raises(ValueError):
        c.irradiance_points(np.zeros((5, 2)), np.zeros((5, 2)))
    with pytest.raises(ValueError):
        c.irradiance_points(p, p, stream_ids=np.arange(6))
    with pytest.raises(ValueError):
        c.irradiance_points(p, p, stream_ids=np.zeros((5, 1)))
