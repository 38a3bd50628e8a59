#!/usr/bin/env python3
"""The A/B a refactor is accepted on: the cost tools, parent and new taking turns, judged by the band rule (cost.band).

  python tools/cost_ab.py --parent <libqaray_hip.so> --new <libqaray_hip.so> --rounds 4 [--rows REGEX] [--out FILE] tool [tool ...]

A tool is the name of a script of tools/ and, in the same (quoted) argument, options for it, in which {side} stands for "parent" or
"new": "gpu_ray_query_cost.py --out /tmp/{side}.txt".
Per round and tool: parent, then new, each a process of its own with QA_HIP_LIB naming the side's library, under --limit seconds.
This process never opens the GPU; the first process that fails or runs out of time ends the job, and nothing is run twice.
--parent-tools DIR runs the parent side with the script of the same name from DIR (a folder beside tools/, holding the tools of
the parent commit) and both sides on --new's library: the A/B of a change to the tools themselves; rows of DIR's tools that carry
no id take the id of the new side's row at the same place.

Written to --out and printed: every process's median (min - max) per row id and round; then per row id the rule - parent medians,
new medians, allowed, the new median of N, the verdict, the marks - and "k of n inside".  Exit status 0 only if every row is inside
(2 if one is not, 1 if a process failed).
--rows restricts the rule to the ids the expression matches: the rows that run changed code."""
import argparse
import os
import re
import shlex
import subprocess
import sys

import cost


def triples(rows):
    """row id -> (median, min, max): of the row itself, and of every field that is a summary of its own (id + the field's name)"""
    out = {}
    for r in rows:
        for name, d in [(r["id"], r)] + [(f"{r['id']} {k}", v) for k, v in r.items() if isinstance(v, dict)]:
            if "median_ms" in d and "min_ms" in d and "max_ms" in d:
                out[name] = (d["median_ms"], d["min_ms"], d["max_ms"])
    return out


def run(script, args, lib, limit):
    """One process of one side, its output written through -> its rows"""
    what = f"{script} on {lib}"
    try:
        r = subprocess.run([sys.executable, script, *args], env={**os.environ, "QA_HIP_LIB": lib}, timeout=limit, stdout=subprocess.PIPE, text=True)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"cost_ab: {what} did not finish in {limit} s; nothing more is started")
    print(f"# {what}", flush=True)
    sys.stdout.write(r.stdout)
    if r.returncode != 0:
        raise SystemExit(f"cost_ab: {what} ended with {r.returncode}; nothing more is started")
    return cost.rows_of(r.stdout)


def tables(runs, rounds, pattern):
    """runs: row id -> side -> the triples of its processes in round order -> the lines of the two tables, rows outside"""
    fmt = lambda t: f"{t[0]:.4f} ({t[1]:.4f} - {t[2]:.4f})"   # noqa: E731
    width = max(len(i) for i in runs) + 2
    a = [f"a. Every process: the tool's median (min - max) per row and round, in ms.", "",
         f"{'row':<{width}}{'round':<7}{'parent median (min - max)':<34}new median (min - max)"]
    b = ["", f"b. The rule (cost.band).  allowed: the parent's min - max over its {rounds} processes, or the 3 % band around the median of its {rounds} medians; then the new",
         f"side's median of {rounds}, the verdict, its distance from the parent's, and each of the new side's medians against the same band (. inside, - below, + above).", "",
         f"{'row':<{width}}{'parent medians':<{max(9 * rounds, 14) + 2}}{'new medians':<{max(9 * rounds, 14) + 2}}{'allowed':<32}new median of {rounds}"]
    judged = [i for i in runs if re.search(pattern, i)]
    outside = 0
    for i, sides in runs.items():
        for k in range(rounds):
            a.append(f"{i if k == 0 else '':<{width}}{k + 1:<7}{fmt(sides['parent'][k]):<34}{fmt(sides['new'][k])}")
        if i in judged:
            v = cost.band(sides["parent"], sides["new"])
            outside += v["verdict"] != "inside"
            medians = {s: " ".join(f"{t[0]:.4f}" for t in sides[s]) for s in sides}
            allowed = f"{v['allowed'][0]:.4f} - {v['allowed'][1]:.4f} ({v['kind']:<5})"
            b.append(f"{i:<{width}}{medians['parent']:<{max(9 * rounds, 14) + 2}}{medians['new']:<{max(9 * rounds, 14) + 2}}{allowed:<32}"
                     f"{v['new_median']:.4f} {v['verdict']} {v['percent']:+.1f} %  [{v['marks']}]")
    b.append(f"{len(judged) - outside} of {len(judged)} inside")
    return a + b, outside


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", help="the parent's library (not needed with --parent-tools)")
    ap.add_argument("--new", required=True, help="the new library")
    ap.add_argument("--parent-tools", help="a folder with the parent commit's tools: the A/B is of the tools, both sides on --new")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--rows", default="", help="the rule is applied to the row ids this expression matches (default: all)")
    ap.add_argument("--limit", type=int, default=4 * 240 + 60,
                    help="seconds one process of a tool may take (default: four children, the most a tool starts, of 240 s each, and a minute to start up)")
    ap.add_argument("--out")
    ap.add_argument("tool", nargs="+")
    a = ap.parse_args()
    if not (a.parent or a.parent_tools):
        ap.error("--parent or --parent-tools")
    new_lib = os.path.abspath(a.new)
    runs = {}
    for k in range(a.rounds):
        for tool in a.tool:
            name, *args = shlex.split(tool)
            name = os.path.basename(name if name.endswith(".py") else name + ".py")
            sides = {"parent": (a.parent_tools or os.path.join(cost.ROOT, "tools"), new_lib if a.parent_tools else os.path.abspath(a.parent or "")),
                     "new": (os.path.join(cost.ROOT, "tools"), new_lib)}
            rows = {side: run(os.path.join(folder, name), [x.replace("{side}", side) for x in args], lib, a.limit) for side, (folder, lib) in sides.items()}
            if [r.get("id") for r in rows["parent"]] != [r["id"] for r in rows["new"]]:
                if not a.parent_tools or len(rows["parent"]) != len(rows["new"]):
                    raise SystemExit(f"cost_ab: {name}: the two sides' rows differ; nothing more is started")
                rows["parent"] = [{"id": n["id"], **p} for p, n in zip(rows["parent"], rows["new"])]
            for side in rows:
                for i, t in triples(rows[side]).items():
                    runs.setdefault(f"{name[len('gpu_'):-len('_cost.py')]} {i}", {"parent": [], "new": []})[side].append(t)
    lines, outside = tables(runs, a.rounds, a.rows)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    sys.exit(2 if outside else 0)


if __name__ == "__main__":
    main()
