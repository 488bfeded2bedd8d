#!/usr/bin/env python3
"""Static instruction counts of a kernel's gfx950 assembly, per category.

    hipcc --offload-arch=gfx950 ... --save-temps -c coeb_extract.hip
    tools/isa_count.py coeb_extract-hip-amdgcn-amd-amdhsa-gfx950.s k_blur_rows          # whole kernel + blocks
    tools/isa_count.py FILE.s k_blur_rows 120 260                                     # kernel lines [120, 260)

With a kernel name only: the totals, then one line per basic block (label, first line relative
to the kernel's entry, counts), so that the blocks of a region can be picked out and summed
with a line range.  Categories (profiles/r07/isa_counts.md):
  valu    v_* except the exec-mask writers below
  salu    s_* except waits, branches and exec-mask save / restore
  wait    s_waitcnt*, s_nop
  lds     ds_*
  vmem    buffer_*, global_*, flat_*, scratch_*
  smem    s_load_*, s_buffer_load_*
  branch  s_branch, s_cbranch_*, s_endpgm
  exec    instructions that write exec (s_*saveexec*, s_* exec, ..., v_cmpx_*)
"""
import re
import sys

CATS = ("valu", "salu", "wait", "lds", "vmem", "smem", "branch", "exec")


def category(line):
    t = line.split()
    op = t[0]
    if op.startswith("s_waitcnt") or op == "s_nop":
        return "wait"
    if op in ("s_branch", "s_endpgm") or op.startswith("s_cbranch"):
        return "branch"
    if op.startswith("s_load_") or op.startswith("s_buffer_load_"):
        return "smem"
    if "saveexec" in op or op.startswith("v_cmpx") or (op.startswith("s_") and len(t) > 1 and t[1].rstrip(",") == "exec"):
        return "exec"
    if op.startswith("ds_"):
        return "lds"
    if op.split("_")[0] in ("buffer", "global", "flat", "scratch"):
        return "vmem"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("s_"):
        return "salu"
    return None


def kernel_lines(path, name):
    out, on = [], False
    for ln in open(path):
        if not on:
            if re.match(r"^_Z\w*%s\w*:" % re.escape(name), ln):
                on = True
            continue
        if ln.startswith(".Lfunc_end"):
            break
        out.append(ln.rstrip("\n"))
    if not out:
        sys.exit("kernel %s not found in %s" % (name, path))
    return out


def count(lines):
    c = dict.fromkeys(CATS, 0)
    for ln in lines:
        s = ln.strip()
        if not s or s.startswith(";") or s.startswith(".") or s.endswith(":") or re.match(r"^\.?\w+:", s):
            continue
        k = category(s)
        if k:
            c[k] += 1
    return c


def fmt(c):
    return " ".join("%s=%d" % (k, c[k]) for k in CATS) + " total=%d" % sum(c.values())


def main():
    path, name = sys.argv[1], sys.argv[2]
    lines = kernel_lines(path, name)
    if len(sys.argv) >= 5:
        a, b = int(sys.argv[3]), int(sys.argv[4])
        print("%s [%d, %d): %s" % (name, a, b, fmt(count(lines[a:b]))))
        return
    print("%s: %s" % (name, fmt(count(lines))))
    start, label = 0, "entry"
    for i, ln in enumerate(lines + [".Lend:"]):
        m = re.match(r"^(\.L\w+):", ln)
        if m:
            c = count(lines[start:i])
            if sum(c.values()):
                print("  %-12s @%-5d %s" % (label, start, fmt(c)))
            start, label = i, m.group(1)


if __name__ == "__main__":
    main()
