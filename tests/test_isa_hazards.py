"""The compiler hazard behind the photon-walk nondeterminism of rounds 1 / 2 (profiles/round03/photon_walk_root_cause.txt):
hipcc placed a register-allocator spill STORE at the head of a control-flow join block, ahead of the `s_or_b64 exec, exec, ...` that
re-enables the lanes which skipped the preceding divergent region; those lanes never stored, and the matching reload replaced their good
register contents by whatever the scratch slot held.  The build keeps the gfx950 assembly of every translation unit (-save-temps=obj);
no shipped kernel may contain that pattern, and the checker must find it in the excerpt of the kernel that did."""
import glob
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tools", "isa_exec_spill_check.py")


def _run(path):
    return subprocess.run([sys.executable, CHECK, path], stdout=subprocess.PIPE, text=True).stdout


def test_checker_finds_the_hazard_in_the_kernel_that_had_it():
    out = _run(os.path.join(ROOT, "tests", "golden", "isa", "photon_inline_128vgpr_excerpt.s"))
    assert "total hazardous spill stores: 2" in out, out
    assert ".LBB8_459" in out and "offset:320" in out


def test_shipped_kernels_are_free_of_it():
    files = sorted(glob.glob(os.path.join(ROOT, "qaray_amd", "lib", "obj", "*-hip-amdgcn-amd-amdhsa-gfx950.s")))
    if not files:
        pytest.skip("no assembly next to the objects (run __graft_entry__.build())")
    units = {os.path.basename(f).split("-hip-")[0] for f in files}   # (a partial build must not pass for a whole one)
    sources = {os.path.splitext(os.path.basename(f))[0] for f in glob.glob(os.path.join(ROOT, "qaray_amd", "csrc", "hip", "*.hip"))}
    assert sources <= units, f"units without assembly: {sorted(sources - units)}"
    for f in files:
        out = _run(f)
        assert "total hazardous spill stores: 0" in out, f + "\n" + out[-3000:]


def test_headline_kernel_keeps_its_register_budget():
    """The Cornell-box kernel's speed hangs on its register allocation (five waves per SIMD at 96 registers): a change to
    code it shares with other kernels has cost it 3 % without touching its own text (87 -> 113 spilled registers when shadeSurface's
    statements were reordered for the textured kernels).  The build's object says what the allocation is."""
    objs = [os.path.join(ROOT, "qaray_amd", "lib", "obj", o) for o in ("qa_mega.o", "qa_coop.o")]   # per-lane / cooperative integrators
    if not all(os.path.exists(o) for o in objs):
        pytest.skip("no objects (run __graft_entry__.build())")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), *objs], stdout=subprocess.PIPE, text=True).stdout
    line = [l for l in out.splitlines() if l.rstrip().endswith("qa::qa_integrate<true, false, false, false, false, false>")]
    assert line, out[-2000:]
    vgpr, agpr, sgpr, vspill = (int(x) for x in line[0].split()[:4])
    assert vgpr <= 96 and vspill <= 90, line[0]
    # the cooperative kernels of BASELINE C4 / C5 and C3: their scratch must keep fitting the L2 (C4) / not grow
    for name, limit in (("qa::qa_integrate_cs<true, false, false, false, false>", 80), ("qa::qa_integrate_cs<true, true, true, false, false>", 235)):
        line = [l for l in out.splitlines() if l.rstrip().endswith(name)]
        assert line, name
        vgpr, agpr, sgpr, vspill = (int(x) for x in line[0].split()[:4])
        assert vgpr <= 128 and vspill <= limit, line[0]
