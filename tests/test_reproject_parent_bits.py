"""The three host forms of the reprojection (qa_test_reproject_host, qa_test_reproject_motion_host, qa_test_reproject_moments_host)
against the bits they had before the three forms were folded into one rank-templated source: a SHA-256 per output plane, recorded
in tests/golden/reproject_parent_bits.json at the commit that file names.  The other tests hold the device to the host build and the
host build to a float64 restatement within its tolerance; inside that tolerance all of them could move together, and this one
would see it.  The host library is built with -ffp-contract=off -fno-fast-math: the digests do not depend on the optimiser.  No GPU.

Run this file as a program to record the digests anew (only where a change of the outputs is meant):
    python tests/test_reproject_parent_bits.py"""
import hashlib
import json
import os

import numpy as np
import pytest

import conftest  # noqa: F401  (first: it puts the repository on sys.path when this file runs as a program)
import parent_bits_util as pb
import reproject_motion_util as mu
import reproject_util as ru
from qaray_amd import hip
from reproject_moments_util import call_moments, moments_inputs
from reproject_util import H, W
from test_gpu_reproject_moments import FLAGS as MOMENTS_FLAGS
from test_gpu_reproject_motion import FLAGS as MOTION_FLAGS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reproject_parent_bits.json")
PLANES = ("out", "length", "moments", "variance")


def cases():
    """(name, thunk -> the call's output planes), in a fixed order: the plain form on inputs() at two sizes, still and moving, with
    and without ids, and on every edge case; the motion form over the device test's FLAGS and flags 0; the moments form over its
    device test's FLAGS and both new flags off (the last two forms under a moving and a still camera)."""
    out = []
    for size, origin in (((W, H), (0, 0)), ((62, 42), (5, 3))):
        for still in (False, True):
            for ids in (True, False):
                out.append((f"plain {size[0]}x{size[1]} at {origin} still={still} ids={ids}",
                            lambda size=size, origin=origin, still=still, ids=ids:
                            ru.call(hip.reproject_host, ru.inputs(size[0], size[1], origin, still=still), ids)))
    for name, a in ru.edge_cases():
        out.append((f"plain edge: {name}", lambda a=a: ru.call(hip.reproject_host, a)))
    for still in (False, True):
        for flags in (dict(motion=False),) + tuple(MOTION_FLAGS):
            out.append((f"motion still={still} {json.dumps(flags, sort_keys=True)}",
                        lambda still=still, flags=flags: mu.call_motion(hip.reproject_motion_host, mu.motion_inputs(still=still), **flags)))
        for flags in (dict(moments=False, shorten=False),) + tuple(MOMENTS_FLAGS):
            out.append((f"moments still={still} {json.dumps(flags, sort_keys=True)}",
                        lambda still=still, flags=flags: call_moments(hip.reproject_moments_host, moments_inputs(still=still), **flags)))
    return out


def digests(planes):
    """-> dict plane name -> SHA-256 of its bytes ("none" for a plane the call did not write)."""
    return {name: "none" if a is None else hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest() for name, a in zip(PLANES, planes)}


def record(commit):
    return pb.save(GOLDEN, commit, "SHA-256 of every output plane of hip.reproject_host / reproject_motion_host / reproject_moments_host over cases() of "
                   "tests/test_reproject_parent_bits.py, taken with the library built from that commit", {name: digests(thunk()) for name, thunk in cases()})


def test_the_record_names_every_case_and_nothing_else():
    assert pb.names_match(GOLDEN, [name for name, _ in cases()])


@pytest.mark.parametrize("name,thunk", cases(), ids=[n for n, _ in cases()])
def test_host_forms_keep_the_parents_bits(name, thunk):
    assert digests(thunk()) == pb.load(GOLDEN)[name], name


if __name__ == "__main__":
    pb.main(record)
