#!/usr/bin/env python3
"""Developer helper: compare the device code of two builds of one translation unit, kernel by kernel.

    hipcc <the Makefile's CXXFLAGS> [-DPCR_DEV=1] -S --cuda-device-only csrc/kernels.hip -o old.s   (at the old revision)
    ... the same at the new revision -> new.s
    tools/isa_diff.py old.s new.s [--allow NAME_SUBSTRING ...]

Per kernel: the instruction stream (directives and comments dropped, .LBBn_ label numbers normalised) and the resource
fields of its .amdhsa_kernel block.  Exit status 1 when a kernel that is in both files differs and is not --allow-ed;
an allowed kernel may differ but may not use scratch or more registers than before."""
import re
import sys

FIELDS = "next_free_vgpr|next_free_sgpr|private_segment_fixed_size|group_segment_fixed_size"


def load(path):
    text = open(path).read()
    fn, meta = {}, {}
    # (the label line carries a trailing "; -- Begin function" comment on some kernels)
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        body = [l.strip() for l in m.group(2).splitlines()]
        body = [l for l in body if l and not l.startswith((";", ".", "//"))]
        fn[m.group(1)] = [re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\s*;.*$", "", l)) for l in body]
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S | re.M):
        meta[m.group(1)] = {k: int(v) for k, v in re.findall(rf"\.amdhsa_({FIELDS}) (\d+)", m.group(2))}
    assert meta and all(k in fn and fn[k] for k in meta), "a kernel body was not parsed"
    return fn, meta


def main(old, new, allow):
    (a, am), (b, bm) = load(old), load(new)
    gone, came = sorted(set(am) - set(bm)), sorted(set(bm) - set(am))
    both = [k for k in am if k in bm]
    diff = [k for k in both if a[k] != b[k] or am[k] != bm[k]]
    bad = []
    for k in diff:
        ok = any(s in k for s in allow) and bm[k]["private_segment_fixed_size"] == 0 and \
            all(bm[k][f] <= am[k][f] for f in ("next_free_vgpr", "next_free_sgpr"))
        print("DIFF" if ok else "DIFF (not allowed)", k, len(a[k]), "->", len(b[k]), "instructions;", am[k], "->", bm[k])
        if not ok:
            bad.append(k)
    for k in gone:
        print("only in old:", k)
    for k in came:
        print("only in new:", k)
    print(f"{len(am)} kernels -> {len(bm)}: {len(both) - len(diff)} of {len(both)} common kernels identical, "
          f"{len(diff) - len(bad)} differ as allowed, {len(bad)} differ otherwise, {len(gone)} only in old, {len(came)} only in new")
    return 1 if bad else 0


if __name__ == "__main__":
    args = sys.argv[1:]
    allow = []
    while "--allow" in args:
        i = args.index("--allow")
        allow.append(args[i + 1])
        del args[i:i + 2]
    if len(args) != 2:
        sys.exit(__doc__)
    sys.exit(main(args[0], args[1], allow))
