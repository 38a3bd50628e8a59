"""tools/cost.py, the harness of the cost tools: the band rule against the A/B the project recorded by hand
(tests/golden/cost_band_cases.json, transcribed from profiles/denoise_unify_ab.txt 2a / 2b), the child runner's stop rule with
throw-away child scripts, the row emit prints, and that neither importing the module nor a tool's --help opens the GPU.  No GPU."""
import glob
import json
import os
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
sys.path.insert(0, TOOLS)
import cost  # noqa: E402

with open(os.path.join(ROOT, "tests", "golden", "cost_band_cases.json")) as f:
    RECORDED = json.load(f)["rows"]


def test_the_record_holds_the_rows_the_rule_is_checked_on():
    kinds = [r["kind"] for r in RECORDED]
    assert len(RECORDED) >= 6 and kinds.count("range") >= 2 and kinds.count("3 %") >= 2
    row = next(r for r in RECORDED if r["row"] == "gbuffer c2 guided 1")
    assert (row["marks"], row["verdict"]) == ("..+.", "inside")


@pytest.mark.parametrize("row", RECORDED, ids=[r["row"] for r in RECORDED])
def test_band_gives_the_recorded_bounds_verdict_and_marks(row):
    v = cost.band(row["parent"], row["new"])
    assert [f"{x:.4f}" for x in v["allowed"]] == row["allowed"]
    assert (v["kind"], v["verdict"], v["marks"]) == (row["kind"], row["verdict"], row["marks"])


@pytest.mark.parametrize("shift,verdict,marks", [(0.9, "below", "--.-"), (1.1, "above", "++.+")])
def test_band_says_below_and_above(shift, verdict, marks):
    parent = [(1.00, 0.99, 1.01), (1.01, 1.00, 1.02), (0.99, 0.98, 1.00), (1.00, 0.99, 1.02)]     # allowed: 0.98 - 1.02 (range)
    new = [(shift, shift, shift), (shift, shift, shift), (1.0, 1.0, 1.0), (shift, shift, shift)]
    v = cost.band(parent, new)
    assert (v["kind"], v["allowed"], v["verdict"], v["marks"]) == ("range", (0.98, 1.02), verdict, marks)
    assert v["percent"] == pytest.approx(100 * (shift - 1))


CHILD = """
    import json, os, sys, time
    variant = sys.argv[sys.argv.index("--one") + 1]
    here = os.path.dirname(os.path.abspath(__file__))
    open(os.path.join(here, "started_" + variant), "a").write("x")
    print("a line that is no row")
    print(json.dumps({"variant": variant, "passed": sys.argv[1:sys.argv.index("--one")]}), flush=True)
    if variant == "fails":
        sys.exit(3)
    if variant == "sleeps":
        time.sleep(30)
"""


def run(tmp_path, variants, limit, capsys):
    script = tmp_path / "child_tool.py"
    script.write_text(textwrap.dedent(CHILD))
    try:
        rows, stop = cost.run_children(str(script), [[v] for v in variants], ["--repeats", "5"], limit), None
    except SystemExit as e:
        rows, stop = None, str(e)
    started = {v: len((tmp_path / f"started_{v}").read_text()) if (tmp_path / f"started_{v}").exists() else 0 for v in variants}
    return rows, stop, started, capsys.readouterr().out


def test_a_child_that_fails_ends_the_run(tmp_path, capsys):
    rows, stop, started, out = run(tmp_path, ["first", "fails", "third"], 20, capsys)
    assert rows is None and started == {"first": 1, "fails": 1, "third": 0}
    assert stop == "child_tool: fails ended with 3; nothing more is started"
    assert [r["variant"] for r in cost.rows_of(out)] == ["first", "fails"]       # (what the children printed was written through)


def test_a_child_that_runs_out_of_time_ends_the_run(tmp_path, capsys):
    rows, stop, started, out = run(tmp_path, ["first", "sleeps", "third"], 1, capsys)
    assert rows is None and started == {"first": 1, "sleeps": 1, "third": 0}
    assert stop == "child_tool: sleeps did not finish in 1 s; nothing more is started"
    assert [r["variant"] for r in cost.rows_of(out)] == ["first", "sleeps"]


def test_without_a_failure_every_child_runs_once_and_the_rows_come_back_in_order(tmp_path, capsys):
    rows, stop, started, out = run(tmp_path, ["c2", "c5", "third"], 20, capsys)
    assert stop is None and started == {"c2": 1, "c5": 1, "third": 1}
    assert rows == [{"variant": v, "passed": ["--repeats", "5"]} for v in ("c2", "c5", "third")]
    assert out.count("a line that is no row") == 3


def test_emit_prints_one_line_the_given_keys_then_library_tool_id(capsys, monkeypatch):
    import types
    monkeypatch.setitem(sys.modules, "qaray_amd.hip", types.SimpleNamespace(HIP_LIB_PATH=os.path.join(ROOT, "qaray_amd", "lib", "libqaray_hip.so")))
    cost.emit("gpu_x_cost", "c2 4 spp frame", config="c2", size=[1920, 1080], **cost.summary([0.25, 0.125, 0.5]), what="frame")
    out = capsys.readouterr().out
    assert out.endswith("\n") and out.count("\n") == 1
    row = json.loads(out)
    assert list(row) == ["config", "size", "median_ms", "min_ms", "max_ms", "what", "library", "tool", "id"]
    assert row == {"config": "c2", "size": [1920, 1080], "median_ms": 0.25, "min_ms": 0.125, "max_ms": 0.5, "what": "frame",
                   "library": os.path.join("qaray_amd", "lib", "libqaray_hip.so"), "tool": "gpu_x_cost", "id": "c2 4 spp frame"}


def test_importing_the_harness_imports_neither_torch_nor_the_package():
    code = "import sys; sys.path.insert(0, sys.argv[1]); import cost, cost_ab; assert not {'torch', 'qaray_amd'} & set(sys.modules), sorted(sys.modules)"
    subprocess.run([sys.executable, "-c", code, TOOLS], check=True, timeout=60)


@pytest.mark.parametrize("tool", sorted(os.path.basename(p) for p in glob.glob(os.path.join(TOOLS, "gpu_*_cost.py"))) + ["cost_ab.py"])
def test_help_of_every_tool_needs_no_gpu(tool):
    r = subprocess.run([sys.executable, os.path.join(TOOLS, tool), "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert r.returncode == 0 and "--limit" in r.stdout, r.stderr
