"""Why qa_integrate_lastcast carries no Beer-Lambert block (qaray_amd/csrc/hip/qa_kernel_lastcast_body.h, section C): PlanLastCast
admits a scene only where every material's absorption is +0 or -0.  tests/cpp/absorb_identity_check.cpp shows on the host build of
qa_device_math.h that qexpf(-a * z) is 1.0f bit for bit for a = +0 / -0 and finite z > 0, and that t * 1.0f has t's bits; built
stand-alone with AddressSanitizer + UBSan, no GPU.  On the GPU the kernel's frames are compared with the counting kernel's, which is
the general body and keeps the block: tests/test_gpu_last_cast.py, tests/test_gpu_lastcast_straight.py."""
import os
import subprocess

from conftest import ROOT
from test_cast_cost_host import ENV, SAN


def test_beer_lambert_factor_of_a_zero_absorption_is_one(tmp_path):
    exe = str(tmp_path / "absorb_identity_check")
    hip = os.path.join(ROOT, "qaray_amd", "csrc", "hip")
    subprocess.run(["g++", "-std=c++17", *SAN, "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{ROOT}/include", f"-I{hip}",
                    os.path.join(ROOT, "tests", "cpp", "absorb_identity_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], env=ENV, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "absorb_identity_check: clean" in r.stdout, r.stdout[-3000:]
    assert "runtime error" not in r.stdout and "AddressSanitizer" not in r.stdout, r.stdout[-3000:]
