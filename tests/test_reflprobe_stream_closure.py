"""No reflection-probe entry with a stream arrives untested: every function of include/qaray_hip.h named qa_reflprobe_*_device takes a
`void *stream` and is named in the CASES table of tests/test_gpu_reflprobe.py, whose keys are tests of that file, or in its EXEMPT
dict with the reason why there is nothing to order - what tests/test_probe_stream_closure.py and
tests/test_probevis_stream_closure.py ask of the qa_probe_* and qa_probevis_* entries, whose patterns do not match these.  No GPU."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    text = open(os.path.join(ROOT, "include", "qaray_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def reflprobe_entries():
    """-> (the qa_reflprobe* functions the header declares, those of them with a stream argument)"""
    found = [(m.group(1), m.group(2)) for m in re.finditer(r"\bint\s+(qa_\w+)\s*\(([^;{}()]*)\)\s*;", header()) if re.search(r"^qa_reflprobe(_|$)", m.group(1))]
    return [n for n, _ in found], [n for n, args in found if re.search(r"\bvoid\s*\*\s*(hip_)?stream\b", args)]


def test_the_parser_finds_the_entries():
    names, with_stream = reflprobe_entries()
    assert sorted(with_stream) == ["qa_reflprobe_grid_shade_device", "qa_reflprobe_prefilter_device", "qa_reflprobe_shade_device"], with_stream
    assert sorted(names) == sorted(with_stream + ["qa_reflprobe_layout"]), names
    # every device form has a stream: a new one cannot slip past by another spelling of the argument
    assert sorted(n for n in names if n.endswith("_device")) == sorted(with_stream)
    # none of them is an `_irradiance`, `_ao`, `_bake` or `idmatte` entry, or takes a `hip_stream`: those tables belong to other files
    assert not [n for n in names if re.search(r"_irradiance(_|$)|_ao(_|$)|_bake(_|$)|idmatte", n)]
    assert "hip_stream" not in "".join(a for n, a in re.findall(r"\bint\s+(qa_reflprobe\w+)\s*\(([^;{}()]*)\)\s*;", header()))
    # and none is taken for an entry of the two probe families
    assert not [n for n in names if re.search(r"^qa_probe(_|$)|^qa_probevis(_|$)", n)]
    # the test hooks run on the CPU and take no stream
    hooks = re.findall(r"\bint\s+(qa_test_reflprobe_\w+)\s*\(([^;{}()]*)\)\s*;", header())
    assert len(hooks) == 3 and not [n for n, a in hooks if re.search(r"\bvoid\s*\*\s*(hip_)?stream\b", a)]
    assert not [n for n, _ in hooks if re.search(r"^qa_test_probe_|^qa_test_probevis_", n)]


def test_every_entry_with_a_stream_has_a_case_or_a_reason():
    import test_gpu_reflprobe as T   # (importing it needs no GPU: torch and the library are imported by the tests)
    covered = {e for entries in T.CASES.values() for e in entries}
    _, with_stream = reflprobe_entries()
    assert not [e for e in with_stream if e not in covered and e not in T.EXEMPT]
    assert (covered | set(T.EXEMPT)) <= set(with_stream) and not covered & set(T.EXEMPT)
    assert all(callable(getattr(T, name, None)) for name in T.CASES), "every case of the table is a test of the file"
    assert all(isinstance(r, str) and len(r) > 20 for r in T.EXEMPT.values()), "every exemption gives its reason"
    # nothing of this family orders anything: all three are exempt
    assert sorted(T.EXEMPT) == sorted(with_stream) and not T.CASES
