"""Build-time check of INTEGRATION.md section 1 against the reference's own headers (oracle/Makefile `ref`, only where the
reference tree exists): the binding shown there is compiled with those headers, and the tasking declarations that the host
layer mirrors are looked up in the reference's src/tasking/parallel_for.h.  Only the outcome is written, as JSON under
oracle/_ref/; tests/test_host_layer.py reads it, so the test needs no reference tree of its own.

    python3 integration_check.py REF_DIR OUT.json
"""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INTEGRATION_MD = os.path.join(ROOT, "INTEGRATION.md")
PRELUDE = "#include <memory>\n#include <stdexcept>\n#include <vector>\n#include <cmath>\n"
TASKING_DECLS = ("size_t get_num_of_threads();", "void set_num_of_threads(size_t num_of_threads);", "void init();",
                 "void signal_start();", "void signal_stop();", "bool has_stop_signal();",
                 "void parallel_for(size_t start, size_t end, size_t step, std::function<void(size_t)> T);")


def snippet():
    """The C++ block of INTEGRATION.md section 1 (the new src/renderers/Renderer_HIP.cpp of the reference)."""
    text = open(INTEGRATION_MD).read()
    return re.search(r"```cpp\n(// src/renderers/Renderer_HIP\.cpp.*?)```", text, re.S).group(1)


def snippet_sha256():
    return hashlib.sha256(snippet().encode()).hexdigest()


def norm(text):
    return re.sub(r"\s+", " ", text)


def main(ref, out):
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "Renderer_HIP.cpp")
        open(src, "w").write(PRELUDE + snippet())
        inc = [f"-I{ref}/src", f"-I{ref}", f"-I{ref}/external", f"-I{ref}/external/glm", f"-I{ROOT}/include"]
        r = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-w", "-fpermissive", "-DUSE_GLM", "-DUSE_OMP", "-fopenmp", *inc, src],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    ref_h = norm(open(os.path.join(ref, "src", "tasking", "parallel_for.h")).read())
    result = {"snippet_sha256": snippet_sha256(), "compile_rc": r.returncode, "compile_output": r.stdout[-3000:],
              "reference_declares": {d: d in ref_h for d in TASKING_DECLS}}
    with open(out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
