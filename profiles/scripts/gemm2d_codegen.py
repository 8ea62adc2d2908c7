"""Code generation of the 37 kernels of gemm2d.hip, two builds paired kernel by kernel (no GPU).

  python profiles/scripts/gemm2d_codegen.py resources A.txt B.txt
      A.txt / B.txt = stderr of  hipcc <the Makefile's HIPFLAGS> -Rpass-analysis=kernel-resource-usage -c gemm2d.hip
      -> registers, scratch, LDS bytes and occupancy per pair (profiles/gemm2d_one_loop_resources.txt)
  python profiles/scripts/gemm2d_codegen.py loops A.s B.s [MATH SUBSTRING]
      A.s / B.s = hipcc <HIPFLAGS> -S --cuda-device-only gemm2d.hip
      -> per pair: instructions of the whole kernel, then of the part from the first to the last s_barrier (the stage loop and what
         the block layout puts around it), how many of those are s_waitcnt vmcnt, and how many lines of that part differ once
         register numbers and labels are renamed;
         with MATH (fp32-64 | fp32-128 | split) and a substring of the operand list, the unified diff of that pair

Kernels are paired by (math, operands, store) whatever the __global__ templates are called in either build."""
import collections
import difflib
import re
import subprocess
import sys

ORDER = {"fp32-64": 0, "fp32-128": 1, "split": 2, "-": 3}


def demangle(name):
    return subprocess.check_output(["c++filt", name], text=True).strip()


def key(name):
    name = re.sub(r"\(.*$", "", name.replace("toda::", "")).replace("void ", "")
    s2 = "WS2Dgrad, PixS2Dgrad, StoreS2Class"
    if name.startswith("pg_slab_reduce_kernel"):
        return ("-", "slab_reduce")
    if name.startswith("pg_s2_dgrad_split_kernel"):
        return ("split", s2)
    for pat, math in ((r"pg_s2_dgrad_kernel<(\d+)>()", "fp32-{}"), (r"pg_gemm_kernel<(\d+), (.*)>$", "fp32-{}"), (r"pg_gemm_split_kernel<()(.*)>$", "split"),
                      (r"pg_kernel<PgFp32<(\d+)>, (.*)>$", "fp32-{}"), (r"pg_kernel<PgSplit, ()(.*)>$", "split")):
        m = re.match(pat, name)
        if m:
            return (math.format(m.group(1)), m.group(2) or s2)
    raise SystemExit("unparsed kernel name " + name)


def resources(path, key=key):
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(key(demangle(m.group(1))), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+) \[-Rpass", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    return out


def cmd_resources(pa, pb):
    a, b = resources(pa), resources(pb)
    assert set(a) == set(b) and len(a) == 37, (len(a), len(b), set(a) ^ set(b))
    bad = 0
    print(f"{'math':8s} {'operands / store':58s} {'VGPR p->n':>10s} {'AGPR':>7s} {'SGPR p->n':>10s} {'scratch':>7s} {'LDS bytes p->n':>16s} {'occ p->n':>8s}")
    for k in sorted(a, key=lambda k: (ORDER[k[0]], k[1])):
        p, n = a[k], b[k]
        f = lambda x: f"{p[x]}->{n[x]}"
        ok = p["ScratchSize"] == n["ScratchSize"] == "0" and p["LDS Size"] == n["LDS Size"] and p["Occupancy"] == n["Occupancy"]
        bad += not ok
        mark = "" if p["VGPRs"] == n["VGPRs"] else "  (VGPRs moved)"
        print(f"{k[0]:8s} {k[1]:58s} {f('VGPRs'):>10s} {f('AGPRs'):>7s} {f('TotalSGPRs'):>10s} {f('ScratchSize'):>7s} {f('LDS Size'):>16s} {f('Occupancy'):>8s}"
              f"{mark}{'' if ok else '  MISMATCH'}")
    print(f"{len(a)} kernels paired, {bad} with scratch != 0, LDS bytes or occupancy different")
    return 1 if bad else 0


def kernels(path):
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^(_ZN4toda\S+):\s*(;.*)?$", line)
        if m:
            cur = out.setdefault(key(demangle(m.group(1))), [])
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None:
            cur.append(line)
    return out


def renamed(line):
    line = re.sub(r";.*", "", line)
    line = re.sub(r"\.LBB\d+_\d+", "L", line)
    line = re.sub(r"[vsa]\[\d+:\d+\]", "R", line)
    line = re.sub(r"\b[vsa]\d+\b", "r", line)
    return re.sub(r"\s+", " ", line).strip()


def loop(lines):
    bars = [i for i, l in enumerate(lines) if "s_barrier" in l]
    mfma = [i for i, l in enumerate(lines) if "v_mfma" in l]
    return [r for r in map(renamed, lines[bars[0]:max(mfma[-1], bars[-1]) + 1]) if r]


def cmd_loops(pa, pb, show=None):
    a, b = kernels(pa), kernels(pb)
    same = collections.Counter()
    for k in sorted(a, key=lambda k: (ORDER[k[0]], k[1])):
        if k[0] == "-":
            continue
        la, lb = loop(a[k]), loop(b[k])
        ops = difflib.SequenceMatcher(None, la, lb, autojunk=False).get_opcodes()
        d = sum(max(i2 - i1, j2 - j1) for t, i1, i2, j1, j2 in ops if t != "equal")
        same[d == 0] += 1
        wa, wb = (sum(1 for r in map(renamed, x[k]) if r and not r.startswith(".") and not r.endswith(":")) for x in (a, b))
        print(f"{k[0]:8s} {k[1]:55s} kernel {wa:4d}->{wb:4d}  loop {len(la):4d}->{len(lb):4d}  vmcnt waits {sum('vmcnt' in l for l in la)}->{sum('vmcnt' in l for l in lb)}"
              f"  differing loop lines {d}")
    print(f"{same[True]} of {same[True] + same[False]} pairs with the same instruction sequence")
    if show:
        k = [k for k in a if k[0] == show[0] and show[1] in k[1]][0]
        print(k)
        for line in difflib.unified_diff(loop(a[k]), loop(b[k]), lineterm="", n=2):
            print(line)
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "resources":
        sys.exit(cmd_resources(sys.argv[2], sys.argv[3]))
    if len(sys.argv) in (4, 6) and sys.argv[1] == "loops":
        sys.exit(cmd_loops(sys.argv[2], sys.argv[3], sys.argv[4:6] or None))
    sys.exit(__doc__)
