#!/usr/bin/env python3
"""What a host form costs end to end (the carver): Context.cast_rays - staging, copies up, the cast, copies back,
synchronise - of the first n camera rays of bench.py's C2 frame (Cornell box, 1920x1080), all four outputs, at n = 1 (the call's
fixed cost: the host's share shows here) and n = 2^20 (the copies' share).  Wall-clock milliseconds per call: warm-up calls, then the
median of --repeats calls.  Each n runs in a child process of its own under a time limit (--limit seconds), by the rule of
tools/cost.py; tools/cost_ab.py runs this tool on two libraries in turn.  The lines are printed and written to --out (default
profiles/host_stage_cost_rows.txt).  Needs a GPU: there is no fallback."""
import json
import os
import sys

import cost

TOOL = "gpu_host_stage_cost"
COUNTS = ("1", "1048576")


def measure(n, warmup, repeats):
    ctx, _, region, _, _ = cost.open_scene(TOOL, "c2")
    o, d = ctx.camera_rays(region)
    o, d = o[:n].copy(), d[:n].copy()
    spans = cost.walls(lambda k: ctx.cast_rays(o, d), warmup, repeats)
    cost.emit(TOOL, f"cast_rays host n={n}", rays=n, what="cast_rays (host form)", **cost.summary(spans), kernel=ctx.kernel_name())
    ctx.close()


def main():
    ap = cost.arguments(__doc__, repeats=31, one=COUNTS)
    ap.add_argument("--out", default=os.path.join(cost.ROOT, "profiles", "host_stage_cost_rows.txt"))
    a = ap.parse_args()
    if a.one:
        return measure(int(a.one), a.warmup, a.repeats)
    rows = cost.run_children(__file__, [[n] for n in COUNTS], sys.argv[1:], a.limit)
    lines = [f"# tools/gpu_host_stage_cost.py (wall clock per call: median of {a.repeats} calls after {a.warmup} warm-ups), one run on one MI355X"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines + [json.dumps(row) for row in rows]) + "\n")


if __name__ == "__main__":
    main()
