"""Instruction streams of one translation unit's gfx950 kernels at two commits, side by side: what a refactor that must keep the
kernels' bits and speed shows first.  Input: the two directories that `hipcc <the Makefile's flags> -c -save-temps
-Rpass-analysis=kernel-resource-usage -o UNIT.o UNIT.hip 2> UNIT.resource_usage.txt` left (make asm does this per unit).  Per
kernel the instruction lines of the .s are taken — comments, directives, labels and the numbers of local labels dropped — and
compared as text; nothing is looked for in them.  One line per kernel (name, instructions before, after, identical / differs); for a
kernel that differs, the resource remarks of both sides, the lines removed and added — also with the register numbers masked, which
tells renamed registers from other code — and the unified diff of the two streams, its first MAX_DIFF lines (0: all of it).
usage: python tools/isa_compare.py UNIT BEFORE_DIR AFTER_DIR [MAX_DIFF] > profiles/refactor/UNIT_isa.txt      (MAX_DIFF: default 40)"""
import difflib
import os
import re
import subprocess
import sys


def kernels(path):
    """{symbol: [instruction lines]} of the functions that the file declares as kernels"""
    text = open(path).read()
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    out, cur = {}, None
    for line in text.splitlines():
        line = line.split(";")[0].rstrip()
        m = re.match(r"^(\w+):", line)
        if m:
            cur = m.group(1) if m.group(1) in names else None
            if cur:
                out[cur] = []
            continue
        s = line.strip()
        if cur is None or not s or s.startswith(".") or s.endswith(":"):
            if s.startswith(".Lfunc_end"):
                cur = None
            continue
        out[cur].append(re.sub(r"\.LBB\d+_\d+", ".LBB", re.sub(r"\s+", " ", s)))
    return out


def resources(path):
    """{symbol: [remark lines]} of the compiler's kernel-resource-usage remarks"""
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark: [^ ]+ +(.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        body = m.group(1).strip()
        if body.startswith("Function Name:"):
            cur = body.split(":", 1)[1].strip()
            out[cur] = []
        elif cur:
            out[cur].append(body)
    return out


def demangle(sym):
    try:
        return subprocess.run(["c++filt", sym], stdout=subprocess.PIPE, text=True, check=True).stdout.strip().split("(")[0]
    except (OSError, subprocess.CalledProcessError):
        return sym


def changed(a, b):
    """(lines removed, lines added) between two streams"""
    ops = [l[0] for l in difflib.unified_diff(a, b, lineterm="", n=0) if l[:1] in "+-" and l[:3] not in ("+++", "---")]
    return ops.count("-"), ops.count("+")


def main(unit, before, after, max_diff=40):
    s = f"{unit}-hip-amdgcn-amd-amdhsa-gfx950.s"
    a, b = kernels(os.path.join(before, s)), kernels(os.path.join(after, s))
    ra, rb = (resources(os.path.join(d, f"{unit}.resource_usage.txt")) for d in (before, after))
    differing = []
    print(f"# {unit}: kernel, instructions before, after")
    for sym in sorted(set(a) | set(b), key=demangle):
        same = a.get(sym) == b.get(sym)
        print(f"{demangle(sym):60s} {len(a.get(sym, [])):6d} {len(b.get(sym, [])):6d}  {'identical' if same else 'differs'}")
        if not same:
            differing.append(sym)
    for sym in differing:
        print(f"\n## {demangle(sym)}")
        for side, r in (("before", ra), ("after", rb)):
            print(f"{side}: " + "; ".join(r.get(sym, ["(absent)"])))
        x, y = a.get(sym, []), b.get(sym, [])
        mask = lambda lines: [re.sub(r"\b([vsa])(\d+|\[\d+:\d+\])", r"\1#", l) for l in lines]
        print("lines -%d +%d; with register numbers masked -%d +%d" % (changed(x, y) + changed(mask(x), mask(y))))
        diff = list(difflib.unified_diff(x, y, "before", "after", lineterm="", n=0))
        shown = diff[:max_diff] if max_diff else diff
        print("\n".join(shown))
        if len(shown) < len(diff):
            print(f"... {len(diff) - len(shown)} more lines of this diff not kept here")
    return 0


if __name__ == "__main__":
    if len(sys.argv) not in (4, 5):
        sys.exit(__doc__)
    sys.exit(main(*sys.argv[1:4], *map(int, sys.argv[4:])))
