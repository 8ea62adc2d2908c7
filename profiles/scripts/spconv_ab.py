"""Do two builds of libtoda_hip.so compute the same bits in the sparse gather-GEMMs and weight gradients of spconv.hip / spconv_split.cuh?

  python profiles/scripts/spconv_ab.py run LIB_A LIB_B      the cases below, under both matrix paths
  python profiles/scripts/spconv_ab.py compare DIR_A DIR_B  two directories of .npy files (bench.py --dump-outputs)

`run` starts one fresh child process per library (TODA_HIP_LIB is read when toda_amd.lib is imported); the children write .npy files
to a temporary directory, this process compares them with numpy.array_equal and removes them.  Exit status 1 when anything differs.

Cases (seeded; SubM tables cut from tests/helpers.clustered_sparse, K = 27 and a (3, 1, 1) kernel):
  forward with bias and data gradient of PAIRS at ROWS rows; a permuted `order` at 129 rows; the class-sorted stride-2 data gradient
  of CLASSED; the epilogue's BatchNorm moments of MOMENTS at 129 and 1100 rows, folded and as partials (output, 2 cp results, the
  partial block); the weight gradient of WGRAD on tables of WGRAD_ROWS rows, a dense 6 x 6 x 6 block and a strided table."""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PAIRS = [(5, 16), (16, 16), (16, 32), (24, 48), (32, 32), (32, 64), (64, 32), (64, 64), (64, 128), (128, 64), (128, 128), (32, 128), (128, 32)]
ROWS = [1, 31, 33, 127, 129, 1100]
CLASSED = [(16, 32), (64, 64), (64, 128)]
MOMENTS = [(32, 32), (32, 64), (64, 64), (64, 128)]
WGRAD = [(5, 16), (16, 16), (24, 48), (32, 32), (32, 64), (64, 32), (64, 64), (64, 128), (128, 64), (128, 128)]
WGRAD_ROWS = [1, 17, 65, 300, 1100]
SHAPE, BATCH = [9, 40, 44], 2


def child(out_dir):
    sys.path.insert(0, ROOT)
    import torch

    from tests import helpers as H
    from toda_amd import lib, ops

    print("library", lib.LIB_PATH, flush=True)
    ops.CLASS_DGRAD_MIN_ROWS = 0          # the class-sorted data gradient on a small table
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
    sites, _ = H.clustered_sparse(BATCH, SHAPE, 1400, 1, seed=7)
    assert len(sites) >= max(ROWS)
    dense = np.array([[0, z, y, x] for z in range(6) for y in range(6) for x in range(6)], np.int32)
    rng = np.random.default_rng(11)

    def save(name, t):
        np.save(os.path.join(out_dir, name + ".npy"), t.cpu().numpy())

    def operands(cin, cout, ks, n_in, n_out):
        w = (rng.standard_normal((cout,) + ks + (cin,)) / np.sqrt(ks[0] * ks[1] * ks[2] * cin)).astype(np.float32)
        return (dev(rng.standard_normal((n_in, cin)).astype(np.float32)), dev(w), dev(rng.standard_normal(cout).astype(np.float32)),
                dev(rng.standard_normal((n_out, cout)).astype(np.float32)))

    subm = {(n, ks): ops.build_subm_rulebook(dev(sites[:n]), BATCH, SHAPE, ksize=ks)[0] for n in sorted(set(ROWS + WGRAD_ROWS)) for ks in ((3, 3, 3), (3, 1, 1))}
    subm_dense = ops.build_subm_rulebook(dev(dense), 1, [6, 6, 6])[0]
    strided = ops.build_conv_rulebook(dev(sites[:1100]), BATCH, SHAPE, 3, 2, 1)[2]
    perm = dev(np.random.default_rng(5).permutation(129).astype(np.int32))
    for path in ("native", "split"):
        ops.set_matrix_path(path)
        for cin, cout in PAIRS:
            for (n, ks), rb in subm.items():
                if n not in ROWS:
                    continue
                x, w, b, g = operands(cin, cout, ks, n, n)
                tag = f"{path}_{cin}x{cout}_k{ks[1]}_n{n}"
                wf, wd = ops.pack_weight(w, False, False), ops.pack_weight(w, True, True)
                save(tag + "_fwd", ops.gather_gemm(x, wf, rb.nbr_fwd, cout, b))
                save(tag + "_dgrad", ops.gather_gemm(g, wd, rb.nbr_bwd, cin))
                if n == 129:
                    save(tag + "_fwd_perm", ops.gather_gemm(x, wf, rb.nbr_fwd, cout, b, order=perm))
        for cin, cout in CLASSED:
            x, w, b, g = operands(cin, cout, (3, 3, 3), strided.n_in, strided.n_out)
            order, cls = strided.class_order()
            save(f"{path}_{cin}x{cout}_classed_dgrad", ops.gather_gemm_classed(g, ops.pack_weight(w, True, strided.flip_bwd), strided.nbr_bwd, cin, order, cls,
                                                                               strided.ksize, strided.geom["stride"], strided.geom["padding"]))
        for cin, cout in MOMENTS:
            assert ops.gather_gemm_stats_supported(cin, cout)
            for n in (129, 1100):
                rb = subm[(n, (3, 3, 3))]
                x, w, b, g = operands(cin, cout, (3, 3, 3), n, n)
                wf = ops.pack_weight(w, False, False)
                tag = f"{path}_{cin}x{cout}_n{n}_moments"
                out, sums = ops.gather_gemm_with_stats(x, wf, rb.nbr_fwd, cout, b)
                save(tag + "_out", out), save(tag + "_sums", sums[:2 * cout])
                out, sums, blocks = ops.gather_gemm_with_stats(x, wf, rb.nbr_fwd, cout, b, partials=True)
                assert blocks > 0
                save(tag + "_partials_out", out), save(tag + "_partials", sums[2 * cout:2 * cout * (1 + blocks)])
        for cin, cout in WGRAD:
            tables = [(f"n{n}", subm[(n, (3, 3, 3))]) for n in WGRAD_ROWS] + [("dense216", subm_dense), ("strided", strided)]
            for name, rb in tables:
                x, w, b, g = operands(cin, cout, (3, 3, 3), rb.n_in, rb.n_out)
                save(f"{path}_{cin}x{cout}_{name}_wgrad", ops.wgrad(x, g, rb.nbr_fwd, tuple(w.shape)))
    print("arrays written:", len(os.listdir(out_dir)), flush=True)


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
    tmp = tempfile.mkdtemp(prefix="spconv_ab_")
    try:
        dirs = []
        for tag, path in (("a", lib_a), ("b", lib_b)):
            d = os.path.join(tmp, tag)
            os.makedirs(d)
            subprocess.run([sys.executable, os.path.abspath(__file__), "child", d], env=dict(os.environ, TODA_HIP_LIB=os.path.abspath(path)),
                           check=True, timeout=600)
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
