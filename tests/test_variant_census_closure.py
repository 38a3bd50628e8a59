"""The census table of tests/test_gpu_variant_census.py against the built objects (no GPU): its rows name exactly the integrator
kernels that qa_mega.o, qa_coop.o, qa_photon.o and qa_wf.o hold.  A variant added to a picker without a census row fails here."""
import os
import sys

import pytest

from test_gpu_variant_census import ROWS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "qaray_amd", "lib", "obj")
OBJECTS = ("qa_mega.o", "qa_coop.o", "qa_photon.o", "qa_wf.o")   # the units that include the kernel headers


def _shipped_integrators():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from kernel_resources import demangle, kernels_of
    finally:
        sys.path.pop(0)
    names = []
    for o in OBJECTS:
        names += demangle([k["name"] for k in kernels_of(os.path.join(OBJ, o))])
    out = set()
    for n in names:
        n = n[len("void "):] if n.startswith("void ") else n
        n = n.split("(")[0]
        if n.startswith("qa::qa_integrate") or n.startswith("qa::wf_"):
            out.add(n)
    return out


def test_census_rows_are_exactly_the_shipped_integrator_kernels():
    if not all(os.path.exists(os.path.join(OBJ, o)) for o in OBJECTS):
        pytest.skip("no objects (run __graft_entry__.build())")
    shipped = _shipped_integrators()
    listed = [i for r in ROWS for i in r.instances]
    assert len(listed) == len(set(listed)), "an instance has two census rows"
    assert shipped, "no integrator kernels found in the objects"
    assert not shipped - set(listed), f"shipped without a census row: {sorted(shipped - set(listed))}"
    assert not set(listed) - shipped, f"census rows for kernels that are not shipped: {sorted(set(listed) - shipped)}"
    print(f"{len(ROWS)} census rows cover {len(shipped)} kernels; unreachable: {[(r.instances[0], r.unreachable) for r in ROWS if r.unreachable]}")


def test_census_table_shape():
    """36 megakernel instances, 12 cooperative, 6 resume, both staged logic stages; a row without a scene says why."""
    first = [r.instances[0] for r in ROWS]
    assert sum(i.startswith("qa::qa_integrate<") for i in first) == 36
    assert sum(i.startswith("qa::qa_integrate_cs<") for i in first) == 12
    assert sum(i.startswith("qa::qa_integrate_cs_resume<") for i in first) == 6
    assert {i for i in first if i.startswith("qa::wf_logic")} == {"qa::wf_logic<false>", "qa::wf_logic<true>"}
    for r in ROWS:
        assert (r.scene is None) == bool(r.unreachable), r
        assert r.spp >= 2 and r.spp_max >= r.spp
    assert any(r.spp_max > r.spp for r in ROWS if r.call.startswith("mega")) and any(r.spp_max > r.spp for r in ROWS if r.call == "cs")
