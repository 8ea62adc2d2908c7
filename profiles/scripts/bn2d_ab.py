"""Do two builds of libtoda_hip.so compute the same bits in the BatchNorm2d kernels of bn2d.hip?

  python profiles/scripts/bn2d_ab.py run LIB_A LIB_B      SWEEP, MAPPING_CASES, MISALIGNED (every tensor one float past a 16-byte boundary)
                                                          and SLICE_SHAPES (through toda_bn2d_fwd_into / toda_bn2d_bwd_from) of
                                                          tests/bn2d_cases.py, each with and without a sync workspace and with relu 0 and 1:
                                                          y, save, running_mean, running_var, dx, dgamma, dbeta and the two return codes
  python profiles/scripts/bn2d_ab.py compare DIR_A DIR_B  two directories of .npy files (bench.py --dump-outputs)

`run` starts one fresh child process per library (TODA_HIP_LIB is read when toda_amd.lib is imported); the children write .npy files
to a temporary directory, this process compares them as bit patterns (a NaN equals the same NaN) and removes them.  The calls are
those of tests/test_gpu_bn2d_edges.py (guard bands and the fault word checked after every launch).  Exit status 1 when anything
differs."""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def child(out_dir):
    sys.path.insert(0, ROOT)
    from tests import bn2d_cases as B
    from tests import test_gpu_bn2d_edges as E
    from toda_amd import lib as L

    lib = L.load()
    print("library", L.LIB_PATH, flush=True)
    sync = E.Sync(lib)
    cases = [("sweep", batch, B.SWEEP_C, hw, 0, None) for hw, batch in B.SWEEP]
    cases += [("mapping", batch, c, hw, 0, None) for batch, c, hw in B.MAPPING_CASES]
    cases += [("misaligned", batch, B.SWEEP_C, hw, 1, None) for hw, batch in B.MISALIGNED]
    cases += [("slice", batch, 3, hw, 0, (7, 2)) for batch, hw in B.SLICE_SHAPES]
    for kind, batch, c, hw, off, wide in cases:
        case = B.Case(batch, c, hw)
        for given in (1, 0):
            for relu in (0, 1):
                res = E.run(lib, case, relu, sync if given else None, off, into=wide, frm=wide)
                stem = os.path.join(out_dir, f"{kind}_b{batch}_c{c}_hw{hw}_sync{given}_relu{relu}_")
                np.save(stem + "rc.npy", np.array([res.rc_fwd, res.rc_bwd], np.int32))
                for name in E.OUTPUTS:
                    np.save(stem + name + ".npy", getattr(res, name))
    assert lib.toda_device_fault() == 0, lib.toda_last_error()


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).reshape(-1).view(np.uint8),
                                                                        np.ascontiguousarray(b).reshape(-1).view(np.uint8))


def compare(dir_a, dir_b):
    a, b = sorted(os.listdir(dir_a)), sorted(os.listdir(dir_b))
    if a != b:
        print("file lists differ:", sorted(set(a) ^ set(b)))
        return 1
    differ = [f for f in a if f.endswith(".npy") and not same_bits(np.load(os.path.join(dir_a, f)), np.load(os.path.join(dir_b, f)))]
    for f in differ:
        print("DIFFERS", f)
    print(f"compared {sum(f.endswith('.npy') for f in a)} arrays: {len(differ)} differ (bit patterns)")
    return 1 if differ else 0


def run(lib_a, lib_b):
    tmp = tempfile.mkdtemp(prefix="bn2d_ab_")
    try:
        dirs = []
        for tag, path in (("a", lib_a), ("b", lib_b)):
            d = os.path.join(tmp, tag)
            os.makedirs(d)
            subprocess.run([sys.executable, os.path.abspath(__file__), "child", d], env=dict(os.environ, TODA_HIP_LIB=os.path.abspath(path)),
                           check=True, timeout=900)
            dirs.append(d)
        return compare(*dirs)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "child":
        child(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] in ("run", "compare"):
        sys.exit((run if sys.argv[1] == "run" else compare)(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
