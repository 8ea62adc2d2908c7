"""Code generation of the BatchNorm2d kernels of bn2d.hip, two builds paired kernel by kernel (no GPU).

  python profiles/scripts/bn2d_codegen.py A.txt B.txt
      A.txt / B.txt = stderr of  hipcc <the Makefile's HIPFLAGS> -Rpass-analysis=kernel-resource-usage -c bn2d.hip
      -> registers, scratch, LDS bytes, occupancy and workgroups per CU per pair (profiles/bn2d_one_body_resources.txt)

Kernels are paired by (direction, V, BB, K, RELU), BB = 0 for the per-plane family, whether a build spells that family
bn2d_*_split_kernel<V, K, RELU> or bn2d_*_kernel<V, 0, K, RELU>.  Every kernel of B must have a partner in A; what A builds beyond
that is counted.  Exit status 1 when a pair differs in LDS bytes or workgroups per CU, or gains scratch it did not have.
The parsing is that of gemm2d_codegen.py."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gemm2d_codegen import resources  # noqa: E402


def key(name):
    m = re.match(r"void toda::bn2d_(fwd|bwd)(_split)?_kernel<(\d+), (?:(\d+), )?(\d+), (true|false)>\(", name)
    if not m or bool(m.group(2)) != (m.group(4) is None):
        raise SystemExit("unparsed kernel name " + name)
    return (m.group(1), int(m.group(3)), int(m.group(4) or 0), int(m.group(5)), m.group(6) == "true")


def main(pa, pb):
    a, b = resources(pa, key), resources(pb, key)
    assert set(b) <= set(a), sorted(set(b) - set(a))
    bad = moved = 0
    print(f"{'dir':3s} {'V':>1s} {'BB':>2s} {'K':>2s} {'relu':>4s} {'VGPR p->n':>10s} {'SGPR p->n':>10s} {'scratch p->n':>12s} {'LDS p->n':>10s} {'occ p->n':>8s} {'wg/CU':>5s}")
    for k in sorted(b):
        p, n = a[k], b[k]
        f = lambda x: f"{p[x]}->{n[x]}"                                   # noqa: E731
        wg = [int(r["Occupancy"]) // 4 for r in (p, n)]                   # 16 waves per workgroup over 4 SIMDs
        ok = p["LDS Size"] == n["LDS Size"] and wg[0] == wg[1] and (p["ScratchSize"] != "0" or n["ScratchSize"] == "0")
        bad += not ok
        moved += p["VGPRs"] != n["VGPRs"]
        mark = ("" if p["VGPRs"] == n["VGPRs"] else f"  VGPRs {int(n['VGPRs']) - int(p['VGPRs']):+d}") + \
               ("" if p["ScratchSize"] == n["ScratchSize"] else f"  scratch {int(n['ScratchSize']) - int(p['ScratchSize']):+d}") + \
               ("" if p["Occupancy"] == n["Occupancy"] else "  occupancy moved")
        print(f"{k[0]:3s} {k[1]:1d} {k[2]:2d} {k[3]:2d} {int(k[4]):4d} {f('VGPRs'):>10s} {f('TotalSGPRs'):>10s} {f('ScratchSize'):>12s} {f('LDS Size'):>10s} "
              f"{f('Occupancy'):>8s} {wg[0]}->{wg[1]}{mark}{'' if ok else '  MISMATCH'}")
    print(f"{len(b)} kernels in the new build, all paired; the parent builds {len(a)} ({len(a) - len(b)} that no route launches)")
    print(f"{moved} pairs with other VGPR counts; {bad} pairs with new scratch, other LDS bytes or other workgroups per CU")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]) if len(sys.argv) == 3 else __doc__)
