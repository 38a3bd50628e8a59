"""The staging carver of the queries' host forms on the CPU (qaray_amd/csrc/hip/qa_stage.h): tests/cpp/stage_check.cpp, the layout half
stand-alone under AddressSanitizer + UBSan, over the plane declarations of every host form and every subset of their optional planes.
The program's opening comment lists what it checks.  No GPU."""
import os
import subprocess

from conftest import ROOT


def test_layouts_under_asan_ubsan(tmp_path):
    """Built without any HIP include path or macro: the layout half must stand on its own under a host compiler (nothing is loaded
    into Python under a sanitizer)."""
    from test_sanitizers import ENV, SAN
    exe = str(tmp_path / "stage_check")
    subprocess.run(["g++", "-std=c++17", *SAN, "-Wall", "-Wextra", "-Werror", f"-I{ROOT}/qaray_amd/csrc/hip", os.path.join(ROOT, "tests", "cpp", "stage_check.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], env=ENV, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "stage_check: clean" in r.stdout, r.stdout[-3000:]
    assert "runtime error" not in r.stdout and "AddressSanitizer" not in r.stdout, r.stdout[-3000:]
