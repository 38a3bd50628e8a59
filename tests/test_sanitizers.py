"""AddressSanitizer + UBSan builds of the CPU-side code (the GPU pool does not offer sanitizers):
the host layer driven through its loaders with good and malformed input, the HIP library's scene
builder over every scene and over malformed blobs, and the oracle rendering a small image."""
import os
import subprocess

import numpy as np

from conftest import ROOT, ensure_assets

SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def test_host_layer_under_asan_ubsan(tmp_path):
    host = os.path.join(ROOT, "qaray_amd", "csrc", "host")
    srcs = [os.path.join(host, f) for f in ("xml.cpp", "scene.cpp", "mesh.cpp", "image.cpp", "xmlload.cpp", "framebuffer.cpp")]
    exe = str(tmp_path / "host_sanity")
    cmd = ["g++", "-std=c++17", "-pthread", *SAN, "-ffp-contract=off", f"-I{ROOT}/include", f"-I{host}",
           os.path.join(ROOT, "tests", "cpp", "host_sanity.cpp"), *srcs, "-o", exe]
    subprocess.run(cmd, check=True)
    work = tmp_path / "w"
    work.mkdir()
    r = subprocess.run([exe, os.path.join(ROOT, "scenes"), str(work)], env=ENV, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "host_sanity: clean" in r.stdout, r.stdout[-3000:]
    assert "runtime error" not in r.stdout and "AddressSanitizer" not in r.stdout, r.stdout[-3000:]


# The plan BuildScene makes for the BASELINE configurations C1 - C5 at their frame sizes (the values the upload made before the
# builder was split out of it): LDS residency, the cooperative kernel's limits, the stack, and per mesh the own SAH tree / 4-wide tree
BASELINE_PLANS = [
    ("example_project3_sphere.xml", (256, 256), "resident=1 csFits=0 csCullOk=1 stackNeedMax=1 ldsBytes=23744 useFast= useWide="),
    ("example_project12_box.xml", (1920, 1080), "resident=1 csFits=0 csCullOk=1 stackNeedMax=8 ldsBytes=31520 useFast=1 useWide=0"),
    ("example_project7_object.xml", (1920, 1080), "resident=0 csFits=1 csCullOk=1 stackNeedMax=32 ldsBytes=38912 useFast=000 useWide=111"),
    ("example_project12_caustics_glossy.xml", (3840, 2160), "resident=0 csFits=1 csCullOk=1 stackNeedMax=32 ldsBytes=38912 useFast=0 useWide=1"),
    ("trc_scene_tower.xml", (3840, 2160), "resident=0 csFits=1 csCullOk=1 stackNeedMax=44 ldsBytes=51200 useFast=000 useWide=111"),
]


def test_scene_builder_under_asan_ubsan(tmp_path):
    from qaray_amd.host import load_scene_blob
    hip = os.path.join(ROOT, "qaray_amd", "csrc", "hip")
    exe = str(tmp_path / "scene_build_check")
    subprocess.run(["g++", "-std=c++17", *SAN, "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{ROOT}/include",
                    f"-I{hip}", os.path.join(ROOT, "tests", "cpp", "scene_build_check.cpp"), os.path.join(hip, "qa_scene_build.cpp"), "-o", exe],
                   check=True)
    ensure_assets()

    def run(*args):
        r = subprocess.run([exe, *args], env=ENV, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-3000:]
        assert "runtime error" not in r.stdout and "AddressSanitizer" not in r.stdout, r.stdout[-3000:]
        return r.stdout.splitlines()

    def blob_file(name, size):
        p = str(tmp_path / f"{name}.{size[0]}x{size[1]}.bin")
        load_scene_blob(name, size=size).tofile(p)
        return p

    scenes = sorted(f for f in os.listdir(os.path.join(ROOT, "scenes")) if f.endswith(".xml"))
    lines = run("plan", *[blob_file(n, (40, 30)) for n in scenes])
    assert len(lines) == len(scenes) and all(" rc=0 " in ln for ln in lines), "\n".join(lines)
    lines = run("plan", *[blob_file(n, size) for n, size, _ in BASELINE_PLANS])
    for ln, (name, size, plan) in zip(lines, BASELINE_PLANS):
        assert ln.endswith(" rc=0 " + plan), (name, ln)
    lines = run("malformed", blob_file("custom_textures.xml", (24, 18)))
    assert len(lines) == 16, "\n".join(lines)


def test_oracle_under_asan_ubsan(tmp_path):
    from qaray_amd.host import load_scene_blob
    exe = str(tmp_path / "oracle_san")
    main = tmp_path / "main.c"
    main.write_text('''
#include <stdio.h>
#include <stdlib.h>
#include "qa_oracle.h"
int main(int argc, char **argv) {
  FILE *f = fopen(argv[1], "rb"); fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET);
  void *blob = malloc(n); if (fread(blob, 1, n, f) != (size_t) n) return 3; fclose(f);
  int w = atoi(argv[2]), h = atoi(argv[3]);
  float *rgb = malloc(sizeof(float) * 3 * w * h), *d = malloc(sizeof(float) * w * h);
  uint32_t *ns = malloc(4 * w * h); qa_oracle_counters c;
  int rc = qa_oracle_render(blob, 0, 0, w, h, 2, 2, 5, 0x51A7A7, rgb, d, ns, 2, &c);
  double s = 0; for (int i = 0; i < 3 * w * h; ++i) s += rgb[i];
  printf("rc=%d sum=%.6f samples=%llu\\n", rc, s, (unsigned long long) c.samples);
  free(blob); free(rgb); free(d); free(ns); return rc;
}''')
    subprocess.run(["gcc", "-std=gnu11", *SAN, "-fopenmp", "-ffp-contract=off", f"-I{ROOT}/include", f"-I{ROOT}/oracle",
                    str(main), os.path.join(ROOT, "oracle", "qa_oracle.c"), "-o", exe, "-lm"], check=True)
    for scene, (w, h) in (("custom_textures.xml", (24, 18)), ("custom_softshadow.xml", (12, 9)), ("example_project12_box.xml", (24, 18))):
        blob = load_scene_blob(scene, size=(w, h))
        p = tmp_path / "scene.bin"
        blob.tofile(p)
        r = subprocess.run([exe, str(p), str(w), str(h)], env=ENV, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0 and "rc=0" in r.stdout, r.stdout[-3000:]
        assert "runtime error" not in r.stdout and "AddressSanitizer" not in r.stdout, r.stdout[-3000:]
