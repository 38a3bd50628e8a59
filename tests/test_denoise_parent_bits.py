"""The three host forms of the denoiser (qa_test_denoise_host, qa_test_denoise_guided_host, qa_test_denoise_variance_host) against
the bits they had before the three forms were folded into one iteration function, one check and one launch: a SHA-256 per output,
recorded in tests/golden/denoise_parent_bits.json at the commit that file names.  The other tests hold the device to the host build
and the host build to a float64 restatement within its tolerance; inside that tolerance all of them could move together, and this
one would see it.  The host library is built with -ffp-contract=off -fno-fast-math: the digests do not depend on the optimiser.
No GPU.

Run this file as a program to record the digests anew (only where a change of the outputs is meant):
    python tests/test_denoise_parent_bits.py"""
import hashlib
import os

import numpy as np
import pytest

import conftest  # noqa: F401  (first: it puts the repository on sys.path when this file runs as a program)
import parent_bits_util as pb
from denoise_guided_util import GUIDED_SIZES, guided_frame
from denoise_util import HOST_SIZES, random_frame
from denoise_variance_util import VARIANCE_SIZES, variance_frame
from qaray_amd import hip

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "denoise_parent_bits.json")
GUIDES = (("none", False, False), ("normal", True, False), ("albedo", False, True), ("both", True, True))


def _plain(w, h, iterations):
    return hip.denoise_host(*random_frame(w, h, 100 * w + h), iterations=iterations)


def _guided(w, h, use_n, use_a, iterations):
    rgb, depth, ns, normal, albedo = guided_frame(w, h, 100 * w + h)
    return hip.denoise_guided_host(rgb, depth, ns, normal if use_n else None, albedo if use_a else None, iterations=iterations)


def _variance(w, h, use_n, use_a, plane, iterations, scale):
    rgb, depth, ns, normal, albedo, var = variance_frame(w, h, 100 * w + h)
    var = {"given": var, "None": None, "all -1": np.full_like(var, -1)}[plane]
    return hip.denoise_variance_host(rgb, depth, ns, normal if use_n else None, albedo if use_a else None, var, iterations=iterations,
                                     variance_scale=scale)


def cases():
    """(name, thunk -> the call's output), in a fixed order: the plain form on random_frame at every host size and iteration count;
    the guided form on guided_frame at every size, with every set of guides, and unfiltered with both; the variance form on
    variance_frame at every size with no, both and one guide, the plane given, absent and saying "none" everywhere."""
    out = []
    for w, h in HOST_SIZES:
        for it in (0, 1, 2, 3, 5, 6):
            out.append((f"plain {w}x{h} iterations={it}", lambda w=w, h=h, it=it: _plain(w, h, it)))
    for w, h in GUIDED_SIZES:
        for name, use_n, use_a in GUIDES:
            for it in (1, 3, 5):
                out.append((f"guided {w}x{h} guides={name} iterations={it}", lambda w=w, h=h, n=use_n, a=use_a, it=it: _guided(w, h, n, a, it)))
        out.append((f"guided {w}x{h} guides=both iterations=0", lambda w=w, h=h: _guided(w, h, True, True, 0)))
    for w, h in VARIANCE_SIZES:
        for name, use_n, use_a in (GUIDES[0], GUIDES[3], GUIDES[2]):
            for plane in ("given", "None", "all -1"):
                for it, scale in ((1, 4.0), (3, 0.5), (5, 4.0)):
                    out.append((f"variance {w}x{h} guides={name} plane={plane} iterations={it} scale={scale}",
                                lambda w=w, h=h, n=use_n, a=use_a, plane=plane, it=it, scale=scale: _variance(w, h, n, a, plane, it, scale)))
    return out


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float32).tobytes()).hexdigest()


def record(commit):
    return pb.save(GOLDEN, commit, "SHA-256 of the output of hip.denoise_host / denoise_guided_host / denoise_variance_host over cases() of "
                   "tests/test_denoise_parent_bits.py, taken with the library built from that commit", {name: digest(thunk()) for name, thunk in cases()})


def test_the_record_names_every_case_and_nothing_else():
    assert pb.names_match(GOLDEN, [name for name, _ in cases()])


@pytest.mark.parametrize("name,thunk", cases(), ids=[n for n, _ in cases()])
def test_host_forms_keep_the_parents_bits(name, thunk):
    assert digest(thunk()) == pb.load(GOLDEN)[name], name


if __name__ == "__main__":
    pb.main(record)
