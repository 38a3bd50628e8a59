"""No light-probe entry with a stream arrives untested: every function of include/qaray_hip.h named qa_probe_*_device takes a
`void *stream` and is named in the CASES table of tests/test_gpu_probe_stream_order.py, whose keys are tests of that file, or in its
EXEMPT dict with the reason why there is nothing to order - what tests/test_stream_order_closure.py asks of the entries that take a
`hip_stream`, and tests/test_irradiance_stream_closure.py, tests/test_ao_stream_closure.py and tests/test_bake_stream_closure.py of
theirs.  No GPU."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def probe_entries():
    """-> (the qa_probe* functions the header declares, those of them with a stream argument)"""
    text = open(os.path.join(ROOT, "include", "qaray_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    found = [(m.group(1), m.group(2)) for m in re.finditer(r"\bint\s+(qa_\w+)\s*\(([^;{}()]*)\)\s*;", text) if re.search(r"^qa_probe(_|$)", m.group(1))]
    return [n for n, _ in found], [n for n, args in found if re.search(r"\bvoid\s*\*\s*(hip_)?stream\b", args)]


def test_the_parser_finds_the_entries():
    names, with_stream = probe_entries()
    assert sorted(with_stream) == ["qa_probe_grid_shade_device", "qa_probe_sh_device", "qa_probe_shade_device"], with_stream
    assert sorted(names) == ["qa_probe_grid_shade_device", "qa_probe_params_default", "qa_probe_sh", "qa_probe_sh_device", "qa_probe_shade_device"], names
    # every device form has a stream: a new one cannot slip past by another spelling of the argument
    assert sorted(n for n in names if n.endswith("_device")) == sorted(with_stream)
    # and none of them is an `_irradiance`, `_ao`, `_bake` or `idmatte` entry, or takes a `hip_stream`: those tables belong to other files
    assert not [n for n in names if re.search(r"_irradiance(_|$)|_ao(_|$)|_bake(_|$)|idmatte", n)]
    assert "hip_stream" not in "".join(a for n, a in re.findall(r"\bint\s+(qa_probe\w+)\s*\(([^;{}()]*)\)\s*;", open(os.path.join(ROOT, "include", "qaray_hip.h")).read()))
    # the test hooks run on the CPU and take no stream
    hooks = re.findall(r"\bint\s+(qa_test_probe_\w+)\s*\(([^;{}()]*)\)\s*;", open(os.path.join(ROOT, "include", "qaray_hip.h")).read())
    assert len(hooks) == 4 and not [n for n, a in hooks if re.search(r"\bvoid\s*\*\s*(hip_)?stream\b", a)]


def test_every_entry_with_a_stream_has_a_case_or_a_reason():
    import test_gpu_probe_stream_order as T   # (importing it needs no GPU: torch and the library are imported by the tests)
    covered = {e for entries in T.CASES.values() for e in entries}
    _, with_stream = probe_entries()
    assert not [e for e in with_stream if e not in covered and e not in T.EXEMPT]
    assert (covered | set(T.EXEMPT)) <= set(with_stream) and not covered & set(T.EXEMPT)
    assert all(callable(getattr(T, name, None)) for name in T.CASES), "every case of the table is a test of the file"
    assert all(isinstance(r, str) and len(r) > 20 for r in T.EXEMPT.values()), "every exemption gives its reason"
