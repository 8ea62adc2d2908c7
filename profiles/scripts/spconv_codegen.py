"""Resources of the kernels of one or more .hip files, two builds paired by mangled name (no GPU).

  python profiles/scripts/spconv_codegen.py A.txt B.txt
      A.txt / B.txt = stderr of  hipcc <the Makefile's HIPFLAGS> -Rpass-analysis=kernel-resource-usage -c FILE.hip, for one file
      or several concatenated (the same files on both sides)
      -> registers, scratch, LDS bytes and occupancy per pair
         (spconv.hip: profiles/spconv_shared_resources.txt; rulebook.hip, dynvox.hip, voxel_pool.hip and the other includers of
         scan.cuh: profiles/grid_index_shared_resources.txt)

A kernel whose signature changed pairs by its unmangled name, and the line says so.
Exit status 1 when the sets of names differ or a pair differs in scratch bytes, LDS bytes or occupancy."""
import collections
import re
import subprocess
import sys


def resources(path):
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+) \[-Rpass", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    return out


def short(mangled):
    name = subprocess.check_output(["c++filt", mangled], text=True).strip()
    return re.sub(r"\(.*$", "", name.replace("toda::", "").replace("void ", ""))


def main(pa, pb):
    a, b = resources(pa), resources(pb)
    # a kernel whose signature changed on purpose: the one name left over on each side with the same unmangled name
    only_a, only_b = {short(k): k for k in set(a) - set(b)}, {short(k): k for k in set(b) - set(a)}
    for name in sorted(set(only_a) & set(only_b)):
        print(f"{name}: paired by unmangled name ({only_a[name]} -> {only_b[name]})")
        b[only_a[name]] = b.pop(only_b[name])
    if set(a) != set(b):
        print("kernel names differ:", sorted(set(a) ^ set(b)))
        return 1
    names = {k: short(k) for k in a}
    bad = moved = 0
    print(f"{'kernel':66s} {'VGPR p->n':>10s} {'AGPR':>7s} {'SGPR p->n':>10s} {'scratch p->n':>12s} {'LDS bytes p->n':>16s} {'occ p->n':>8s}")
    for k in sorted(a, key=lambda k: names[k]):
        p, n = a[k], b[k]
        f = lambda x: f"{p[x]}->{n[x]}"
        ok = p["ScratchSize"] == n["ScratchSize"] and p["LDS Size"] == n["LDS Size"] and p["Occupancy"] == n["Occupancy"]
        regs = [x for x in ("VGPRs", "AGPRs", "TotalSGPRs") if p[x] != n[x]]
        bad += not ok
        moved += bool(regs)
        mark = f"  ({', '.join(regs)} moved)" if regs else ""
        print(f"{names[k]:66s} {f('VGPRs'):>10s} {f('AGPRs'):>7s} {f('TotalSGPRs'):>10s} {f('ScratchSize'):>12s} {f('LDS Size'):>16s} {f('Occupancy'):>8s}"
              f"{mark}{'' if ok else '  MISMATCH'}")
    fam = collections.Counter(re.sub(r"<.*$", "", v) for v in names.values())
    print(f"{len(a)} kernels paired by mangled name ({', '.join(f'{v} {k}' for k, v in sorted(fam.items()))})")
    print(f"{sum(p['ScratchSize'] != '0' for p in a.values())} of the parent's kernels have scratch; {bad} pairs differ in scratch, LDS bytes or occupancy; "
          f"{moved} pairs with a register count that moved")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
