"""No entry point with a stream arrives untested: every function of include/qaray_hip.h that takes a `void *hip_stream` is named
in the case table of tests/stream_order_util.py (the cases of tests/test_gpu_stream_order.py), or in its EXEMPT dict with the
reason why there is nothing to order.  No GPU."""
import os
import re

import stream_order_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def entries_with_a_stream():
    text = open(os.path.join(ROOT, "include", "qaray_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    found = [m.group(1) for m in re.finditer(r"\bint\s+(qa_\w+)\s*\(([^;{}()]*)\)\s*;", text) if re.search(r"\bvoid\s*\*\s*hip_stream\b", m.group(2))]
    assert len(found) == len(set(found))
    return found


def test_the_parser_finds_the_entries():
    found = entries_with_a_stream()
    assert "hip_stream" in open(os.path.join(ROOT, "include", "qaray_hip.h")).read()
    for name in ("qa_render_region_device", "qa_gbuffer_region_device", "qa_scene_edit_texels_device", "qa_radiance_rays_device", "qa_progressive_advance"):
        assert name in found
    assert len(found) >= 34, found


def test_every_entry_with_a_stream_has_a_case_or_a_reason():
    covered = {e for entries in U.CASES.values() for e in entries}
    missing = [e for e in entries_with_a_stream() if e not in covered and e not in U.EXEMPT]
    assert not missing, f"entries with a hip_stream that no case of tests/stream_order_util.py names: {missing}"


def test_the_table_names_only_real_entries():
    found = set(entries_with_a_stream())
    named = {e for entries in U.CASES.values() for e in entries} | set(U.EXEMPT)
    assert named <= found, sorted(named - found)
    assert not {e for entries in U.CASES.values() for e in entries} & set(U.EXEMPT), "an entry is both covered and exempt"
    assert all(isinstance(r, str) and len(r) > 20 for r in U.EXEMPT.values()), "every exemption gives its reason"


def test_every_case_of_the_table_is_a_case_of_the_gpu_file():
    import test_gpu_stream_order as T   # (importing it needs no GPU: torch and the library are imported by the cases)
    assert list(T.RUN) == list(U.CASES)
    assert list(U.CASES)[-2:] == ["upload_under_frame", "close_under_frame"], "the lifetime cases run last"
