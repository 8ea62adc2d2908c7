"""Do two builds of libtoda_hip.so compute the same bits in the pixel-GEMMs of gemm2d.hip?

  python profiles/scripts/gemm2d_ab.py run LIB_A LIB_B      every S2_CASES / DECONV_CASES entry of tests/test_gpu_conv2d_edges.py and
                                                            the three shapes of gemm2d_bench.py, under both matrix paths: y, dx, dw
  python profiles/scripts/gemm2d_ab.py compare DIR_A DIR_B  two directories of .npy files (bench.py --dump-outputs)

`run` starts one fresh child process per library (TODA_HIP_LIB is read when toda_amd.lib is imported); the children write .npy files
to a temporary directory, this process compares them with numpy.array_equal and removes them.  Exit status 1 when anything differs."""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
BENCH_SHAPES = [("s2", (2, 128, 256, 188, 188)), ("deconv", (2, 128, 256, 188, 188, 1)), ("deconv", (2, 256, 256, 94, 94, 2))]


def child(out_dir):
    sys.path.insert(0, ROOT)
    from tests import test_gpu_conv2d_edges as T
    from toda_amd import lib, ops

    print("library", lib.LIB_PATH, flush=True)
    cases = [("s2", s) for s in T.S2_CASES] + [("deconv", s) for s in T.DECONV_CASES] + BENCH_SHAPES
    for kind, shape in cases:
        x, wt, gy = T._pg_inputs(kind, shape)
        for path in ("native", "split"):
            ops.set_matrix_path(path)
            for name, t in T._pg_run(ops, kind, shape, x, wt, gy).items():
                np.save(os.path.join(out_dir, f"{path}_{kind}_{'x'.join(map(str, shape))}_{name}.npy"), t.cpu().numpy())


def compare(dir_a, dir_b):
    a, b = sorted(os.listdir(dir_a)), sorted(os.listdir(dir_b))
    if a != b:
        print("file lists differ:", sorted(set(a) ^ set(b)))
        return 1
    differ = [f for f in a if not np.array_equal(np.load(os.path.join(dir_a, f), mmap_mode="r"), np.load(os.path.join(dir_b, f), mmap_mode="r"))]
    for f in differ:
        print("DIFFERS", f)
    print(f"compared {len(a)} arrays: {len(differ)} differ (numpy.array_equal)")
    return 1 if differ else 0


def run(lib_a, lib_b):
    tmp = tempfile.mkdtemp(prefix="gemm2d_ab_")
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
