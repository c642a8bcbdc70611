#!/usr/bin/env python3
"""Are the kernels of two device assembly files (hipcc ... --cuda-device-only -S) the same code?
    python tools/asm_same.py old.s new.s [old_symbol=new_symbol ...]
Either side may be several listings joined with `+` (old.s new_a.s+new_b.s: a unit that was split).
Per kernel: same / DIFF (first differing lines) / gone / new, over the function's text from `name:`
to .Lfunc_end (without comments, blank lines, section / symbol directives, the function's index in
.LBB labels and its own name) and its amdhsa.kernels metadata.  Text only: no instruction is looked
for.  Exit status 1 on any DIFF or any new kernel that no old_symbol=new_symbol names."""
import re
import sys

SKIP = re.compile(r"\s*\.(section|text|type|globl|p2align|weak|protected)\b")
META = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
        "vgpr_spill_count")


def functions(text):
    """{symbol: normalised lines} of every function of the file"""
    out = {}
    for m in re.finditer(r"^([A-Za-z_][\w$.]*):.*?^\.Lfunc_end\d+:", text, re.M | re.S):
        name, lines = m.group(1), []
        for ln in m.group(0).split("\n")[1:-1]:
            ln = re.sub(r"\.LBB\d+_", ".LBB_", ln.split(";")[0]).replace(name, "@").strip()
            if ln and not SKIP.match(ln):
                lines.append(ln)
        out[name] = lines
    return out


def metadata(text):
    """{symbol: {field: value}} from amdhsa.kernels"""
    out = {}
    for block in re.split(r"\n  - ", text[text.index("amdhsa.kernels:"):])[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        found = {k: re.search(rf"\.{k}:\s+(\d+)", block) for k in META}
        if name:
            out[name.group(1)] = {k: int(v.group(1)) if v else None for k, v in found.items()}
    return out


def side(paths):
    """functions and metadata of the listings `a.s+b.s+...` (a unit split into several, or joined)"""
    fns, meta = {}, {}
    for p in paths.split("+"):
        text = open(p).read()
        fns.update(functions(text))
        meta.update(metadata(text))
    return fns, meta


def main():
    rename = dict(a.split("=", 1) for a in sys.argv[3:])
    (fo, mo), (fn, mn) = side(sys.argv[1]), side(sys.argv[2])
    bad, seen = 0, set()
    for name, lo in fo.items():
        to = rename.get(name, name)
        if to not in fn:
            print(f"gone  {name}")
            continue
        seen.add(to)
        ln = fn[to]
        diffs = [f"    line {i}: {x!r} -> {y!r}" for i, (x, y) in enumerate(zip(lo, ln)) if x != y]
        if len(lo) != len(ln):
            diffs.append(f"    {len(lo)} -> {len(ln)} lines")
        a, b = mo.get(name, {}), mn.get(to, {})
        diffs += [f"    {k}: {a.get(k)} -> {b.get(k)}" for k in META if a.get(k) != b.get(k)]
        print(f"{'DIFF' if diffs else 'same'}  {name}" + (f" -> {to}" if to != name else ""))
        print("\n".join(diffs[:6]), end="\n" if diffs else "")
        bad += bool(diffs)
    for name in fn:
        if name not in seen:
            print(f"new   {name}")
            bad += 1
    print(f"{len(fo)} -> {len(fn)} kernels, {bad} differ or are unexpectedly new")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
