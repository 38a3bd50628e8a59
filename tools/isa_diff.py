"""Same machine code?  Compares the gfx950 functions of two builds, body by body (no GPU needed).
   python tools/isa_diff.py <object dir A> <object dir B> [--show]
Reads the *-hip-amdgcn-amd-amdhsa-gfx950.s files the build keeps next to its objects (-save-temps=obj), takes the body of every
.amdhsa_kernel (and of the device functions that were not inlined), normalises the compiler's unit-local labels (.LBB<n>_,
.Lfunc_end<n>, .Ltmp<n>: they number a function by its place in the unit) and reports per demangled name: identical, DIFFERENT, or
present on one side only.  Which unit a kernel lives in does not matter.  Exit status 0 when everything is on both sides and
identical.  --show: every differing line of each pair (- A, + B)."""
import difflib, glob, os, re, subprocess, sys

LABEL = re.compile(r"\.(LBB|Lfunc_end|Lfunc_begin|Ltmp)\d+")


def kernels_of(objdir):
    """{mangled name: set of normalised bodies} over every device assembly file of the directory: the kernels, and the device
    functions they call without inlining (those may be in several units: every copy counts).  A body runs from the function's label
    to its .Lfunc_end, so a kernel's descriptor (registers, scratch, LDS) is part of it."""
    files = sorted(glob.glob(os.path.join(objdir, "*-hip-amdgcn-amd-amdhsa-gfx950.s")))
    if not files:
        sys.exit(f"{objdir}: no *-hip-amdgcn-amd-amdhsa-gfx950.s (build with -save-temps=obj)")
    out, kernels = {}, set()
    for path in files:
        body, name = None, None
        for l in open(path).read().splitlines():
            m = re.match(r"(\S+):\s*; @(\S+)$", l)
            if name is None and m and m.group(1) == m.group(2):
                name, body = m.group(1), []
            elif name is not None and re.match(r"\.Lfunc_end\d+:", l):
                out.setdefault(name, set()).add(tuple(body))
                name = None
            elif name is not None:
                k = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)
                if k:
                    kernels.add(k.group(1))
                l = LABEL.sub(lambda k: "." + k.group(1), l.split(";")[0].rstrip())   # (comments carry unit-local numbers too)
                if l.strip():
                    body.append(l)
        assert name is None, f"{path}: {name} has no end"
    for k in kernels:
        assert len(out[k]) == 1, f"kernel {k} is in two units of {objdir}"
    return out, kernels


def main():
    args = [a for a in sys.argv[1:] if a != "--show"]
    if len(args) != 2:
        sys.exit(__doc__)
    (a, ka), (b, kb) = kernels_of(args[0]), kernels_of(args[1])
    mangled = sorted(set(a) | set(b))
    nice = subprocess.run(["c++filt"], input="\n".join(mangled), stdout=subprocess.PIPE, text=True).stdout.splitlines()
    count = {"identical": 0, "DIFFERENT": 0, "only in A": 0, "only in B": 0}
    for m, n in sorted(zip(mangled, nice), key=lambda mn: mn[1]):
        n = re.sub(r"\(.*$", "", re.sub(r"^void ", "", n))
        what = "only in A" if m not in b else "only in B" if m not in a else "identical" if a[m] == b[m] else "DIFFERENT"
        count[what] += 1
        kind = "kernel" if m in ka | kb else "device function"
        print(f"{what:10s} {n}  ({kind}" + (f", {max(len(x) for x in a[m])} lines)" if what == "identical" else ")"))
        if what == "DIFFERENT" and "--show" in sys.argv:
            x, y = sorted(a[m])[0], sorted(b[m])[0]
            delta = [l for l in difflib.unified_diff(x, y, lineterm="", n=0) if not l.startswith(("---", "+++"))]
            print(f"    {sum(l[0] == '-' for l in delta)} of {len(x)} lines of A against {sum(l[0] == '+' for l in delta)} of {len(y)} of B:")
            print("\n".join("      " + l for l in delta))
    print(", ".join(f"{v} {k}" for k, v in count.items()))
    return 0 if count["identical"] == len(mangled) else 1


if __name__ == "__main__":
    sys.exit(main())
