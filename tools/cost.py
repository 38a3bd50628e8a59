"""What the cost tools (tools/gpu_*_cost.py) share: the frame table, the opening of a scene, the timing loops, the row a tool prints,
the child runner and the band rule of an A/B (tools/cost_ab.py).  A module, not a script; importing it imports neither torch nor
qaray_amd, because the parent process of a tool never opens the GPU: what needs them imports them when called, in a child."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the frames of bench.py's C2 and C5: tag -> scene, width, height
CONFIGS = {"c2": ("example_project12_box.xml", 1920, 1080), "c5": ("trc_scene_tower.xml", 3840, 2160)}
TAGS = tuple(CONFIGS)


def frame(tag):
    """-> scene, width, height of c2 / c5, in either letter case (some tools write C2 / C5)"""
    return CONFIGS[tag.lower()]


# ---- in a child: the GPU, a scene, a frame's tensors

def gpu(tool, root=ROOT):
    """-> torch, qaray_amd.hip of the tree `root`; refuses without a GPU"""
    sys.path.insert(0, root)
    import torch
    from qaray_amd import hip
    if not torch.cuda.is_available():
        raise SystemExit(f"{tool}: no GPU (nothing is measured without one)")
    return torch, hip


def assets(root=ROOT):
    """The stand-in meshes and images some scenes name, generated into the tree's scenes"""
    subprocess.run([sys.executable, os.path.join(root, "scenes", "gen_assets.py")], check=True, stdout=subprocess.DEVNULL)


def open_scene(tool, what, root=ROOT, options=()):
    """A context with a frame uploaded - a tag of CONFIGS or a tool's own (scene, width, height) - after set_option of every (name,
    value) of `options` -> context, blob, region, device, a stream of its own"""
    torch, hip = gpu(tool, root)
    from qaray_amd.host import load_scene_blob
    scene, w, h = frame(what) if isinstance(what, str) else what
    dev = torch.device("cuda", 0)
    ctx = hip.Context(0)
    for name, value in options:
        ctx.set_option(name, value)
    blob = load_scene_blob(scene, size=(w, h))
    ctx.upload_scene(blob)
    return ctx, blob, (0, 0, w, h), dev, torch.cuda.Stream(dev)


def frame_tensors(dev, w, h, ids=False):
    """-> rgb, depth, ns (and ids), uninitialised"""
    import torch
    t = (torch.empty((h, w, 3), dtype=torch.float32, device=dev), torch.empty((h, w), dtype=torch.float32, device=dev),
         torch.empty((h, w), dtype=torch.int32, device=dev))
    return t + ((torch.empty((h, w, 2), dtype=torch.int32, device=dev),) if ids else ())


# ---- timing

def _span(stream, call, launches=1, hold_cycles=0):
    """One window: `launches` calls between two events on `stream`, per call.  With hold_cycles the stream is first held busy
    (torch.cuda._sleep) so that the host - the Python wrapper's checks, the ctypes call, the launcher's occupancy query - runs ahead
    and the calls queue up: the window is then the device's time for them and not the host's latency, which would be a sizeable
    share of a 0.05 ms call."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        if hold_cycles:
            torch.cuda._sleep(hold_cycles)
        e0.record()
        for _ in range(launches):
            call()
        e1.record()
    stream.synchronize()
    return e0.elapsed_time(e1) / launches


def timed(stream, call, warmup, repeats, before=None, launches=1, hold_cycles=0):
    """Event time of `call` on `stream`: warm-up windows, then -> the spans of `repeats` windows in ms.  `before` runs ahead of
    every window, outside it (the stream is drained after it)."""
    spans = []
    for _ in range(warmup + repeats):
        if before:
            before()
            stream.synchronize()
        spans.append(_span(stream, call, launches, hold_cycles))
    return spans[warmup:]


def timed_turns(stream, calls, order, warmup, repeats, after=None):
    """The calls of `order` (names in the dict `calls`) take turns inside every repeat, each between two events of its own;
    after(name) runs behind every call.  -> name -> the spans of `repeats` rounds in ms"""
    spans = {name: [] for name in order}
    for i in range(warmup + repeats):
        for name in order:
            span = _span(stream, calls[name])
            if i >= warmup:
                spans[name].append(span)
            if after:
                after(name)
    return spans


def wall(fn):
    """Wall-clock milliseconds of fn() (which ends in a synchronise where the device's work is meant)"""
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def walls(fn, warmup, repeats):
    """fn(k) for k = 0 .. warmup + repeats - 1 -> the wall-clock ms of the last `repeats`"""
    return [wall(lambda: fn(k)) for k in range(warmup + repeats)][warmup:]


def summary(t, digits=4):
    return {"median_ms": round(statistics.median(t), digits), "min_ms": round(min(t), digits), "max_ms": round(max(t), digits)}


# ---- rows

def library(root=ROOT):
    """The library this process measures, relative to the tree"""
    return os.path.relpath(sys.modules["qaray_amd.hip"].HIP_LIB_PATH, root)


def emit(tool, id, **fields):
    """Print one row: the tool's fields in their order, then the library measured (relative to the tree, unless the tool gave one),
    the tool and the id that names the row within the tool - what an A/B joins on."""
    fields.setdefault("library", library())
    print(json.dumps({**fields, "tool": tool, "id": id}), flush=True)


def rows_of(text):
    return [json.loads(line) for line in text.splitlines() if line.startswith("{")]


# ---- the parent: arguments, children

def arguments(doc, repeats=7, one=None):
    """The parser every tool starts from: --warmup --repeats --limit --one"""
    ap = argparse.ArgumentParser(description=doc, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=repeats)
    ap.add_argument("--limit", type=int, default=240, help="seconds a child process may take")
    ap.add_argument("--one", choices=one, help="measure this configuration in this process" if one else "measure in this process")
    return ap


def run_children(script, variants, passthrough, limit, through=True):
    """The rule the shared machines depend on, once.  Each variant (a list of arguments after --one) is measured by a child process
    of its own under `limit` seconds: python script <passthrough> --one <variant>.  One after the other, so never more than one
    process has the GPU open, and this process never opens it.  The child's output is written through (unless the caller prints
    the rows itself) and its JSON rows are collected -> the rows of all variants in order.  A child that fails or runs out of time
    ends the run with SystemExit; nothing is started after it and no child is started twice."""
    tool = os.path.splitext(os.path.basename(script))[0]
    rows = []
    for variant in variants:
        name = " ".join(variant)
        try:
            r = subprocess.run([sys.executable, os.path.abspath(script), *passthrough, "--one", *variant], timeout=limit, stdout=subprocess.PIPE, text=True)
        except subprocess.TimeoutExpired as e:
            sys.stdout.write(e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else e.stdout or "")
            raise SystemExit(f"{tool}: {name} did not finish in {limit} s; nothing more is started")
        if through or r.returncode != 0:
            sys.stdout.write(r.stdout)
            sys.stdout.flush()
        if r.returncode != 0:
            raise SystemExit(f"{tool}: {name} ended with {r.returncode}; nothing more is started")
        rows += rows_of(r.stdout)
    return rows


# ---- the band rule of an A/B

def band(parent, new):
    """The acceptance rule of a refactor's A/B, for one row id; parent and new are the (median, min, max) of that row in each of
    the side's processes.  As profiles/denoise_unify_ab.txt 2 / 2b states it, and profiles/reproject_unify_ab.txt and
    profiles/firsthit_unify_ab.txt applied it again:

      "over the rounds, a variant's new median (the median of its four processes' medians) must lie within the min - max range the
       parent's build shows for that variant in the same session (over its four processes); a range narrower than 3 % of the
       parent's median is replaced by that median +- 1.5 %."
      "allowed: the parent's min - max over its four processes, or the 3 % band around the median of its four medians; then the
       new build's median of four, the verdict, its distance from the parent's median of four, and in brackets each of the new
       build's four medians against the same band (. inside, - below, + above)."

    -> dict: allowed (lo, hi), kind "range" | "3 %", parent_median, new_median, verdict "inside" | "below" | "above", percent (the new
    median's distance from the parent's), marks (one of . - + per process of the new side)."""
    centre = statistics.median(p[0] for p in parent)
    lo, hi, kind = min(p[1] for p in parent), max(p[2] for p in parent), "range"
    if hi - lo < 0.03 * centre:
        lo, hi, kind = 0.985 * centre, 1.015 * centre, "3 %"

    def where(x):
        return "below" if x < lo else "above" if x > hi else "inside"

    median = statistics.median(n[0] for n in new)
    return {"allowed": (lo, hi), "kind": kind, "parent_median": centre, "new_median": median, "verdict": where(median),
            "percent": 100 * (median / centre - 1), "marks": "".join({"inside": ".", "below": "-", "above": "+"}[where(n[0])] for n in new)}
