"""Time the four BatchNorm2d entry points of bn2d.hip under two builds of libtoda_hip.so, alternating.

  python profiles/scripts/bn2d_bench.py kernels LIB_A LIB_B [RUNS]   child processes A, B, A, B, ... (RUNS of each, default 3); per shape
                                                                      the median over a library's runs and the acceptance verdict
  python profiles/scripts/bn2d_bench.py steps LIB_A LIB_B [RUNS]     the same alternation over bench.py (C3, samples per second)

Shapes: every distinct (entry point, batch, C, hw[, channels of the wider tensor]) that toda_amd/tools/op_table.py recorded for one C3
and one C5 step (profiles/r05_layers_c3.json, profiles/r05_layers_c5.json: the listing does not carry relu, so each is timed with relu 0 and 1),
called with a sync workspace as a training step does; plus, with NO workspace, one shape for each per-channel kernel that spills
(backward V1 BB2 K36, V1 BB4 K18, V4 BB2 K8, V4 BB2 K9, V4 BB4 K4; forward V1 BB2 K36) and forward V4 BB2 K4.
A child times one shape by device events around CALLS back-to-back calls after a warm-up, REPEATS times, and reports the median.
Verdict per shape: B's median over its runs is no worse than A's by more than A's own spread (max - min of its runs' medians)."""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LISTINGS = ("profiles/r05_layers_c3.json", "profiles/r05_layers_c5.json")
NO_WORKSPACE = [("toda_bn2d_bwd", 2, 128, 36863), ("toda_bn2d_bwd", 4, 128, 18431), ("toda_bn2d_bwd", 2, 128, 32400), ("toda_bn2d_bwd", 2, 128, 35344),
                ("toda_bn2d_bwd", 4, 128, 16384), ("toda_bn2d_fwd", 2, 128, 36863), ("toda_bn2d_fwd", 2, 128, 16384)]
CALLS, REPEATS, WARMUP = 50, 9, 20


def shapes():
    out = []
    for path in LISTINGS:
        for row in json.load(open(os.path.join(ROOT, path)))["kernels"]:
            if row["op"].startswith("toda_bn2d_"):
                for relu in (0, 1):
                    s = (row["op"], *row["shape"][:3], relu, (row["shape"] + [0])[3], 1)
                    if s not in out:
                        out.append(s)
    return out + [(op, b, c, hw, relu, 0, 0) for op, b, c, hw in NO_WORKSPACE for relu in (0, 1)]


def child():
    sys.path.insert(0, ROOT)
    import torch

    from toda_amd import lib as L

    lib = L.load()
    ws = torch.zeros((lib.toda_bn2d_sync_bytes(),), dtype=torch.uint8, device="cuda")
    epoch = [0]

    def sync_args(given):
        epoch[0] += 1
        return (L.ptr(ws), epoch[0]) if given else (None, 0)

    result = {}
    for op, b, c, hw, relu, wide, given in shapes():
        g = torch.Generator(device="cuda").manual_seed(1)
        x, dy = (torch.randn((b, c, hw), device="cuda", generator=g) for _ in range(2))
        gamma, beta = torch.rand((c,), device="cuda", generator=g) + 0.5, torch.randn((c,), device="cuda", generator=g)
        rm, rv, save = torch.zeros_like(gamma), torch.ones_like(gamma), torch.empty((2, c), device="cuda")
        y, dx, dgamma, dbeta = torch.empty((b, wide or c, hw), device="cuda"), torch.empty_like(x), torch.empty_like(gamma), torch.empty_like(gamma)
        gwide = torch.randn((b, wide, hw), device="cuda", generator=g) if wide and "bwd" in op else None
        P, st = L.ptr, L.stream()

        def fwd():
            return lib.toda_bn2d_fwd_into(P(x), b, c, hw, P(gamma), P(beta), P(rm), P(rv), 0.01, 1e-3, relu, P(y), wide or c, 0, P(save), *sync_args(given), st)

        call = {"toda_bn2d_fwd": lambda: lib.toda_bn2d_fwd(P(x), b, c, hw, P(gamma), P(beta), P(rm), P(rv), 0.01, 1e-3, relu, P(y), P(save), *sync_args(given), st),
                "toda_bn2d_fwd_into": fwd,
                "toda_bn2d_bwd": lambda: lib.toda_bn2d_bwd(P(x), P(dy), b, c, hw, P(gamma), P(beta), P(save), relu, P(dx), P(dgamma), P(dbeta), *sync_args(given), st),
                "toda_bn2d_bwd_from": lambda: lib.toda_bn2d_bwd_from(P(x), P(gwide), wide, 0, b, c, hw, P(gamma), P(beta), P(save), relu, P(dx), P(dgamma), P(dbeta),
                                                                     *sync_args(given), st)}[op]
        assert fwd() == 0, lib.toda_last_error()          # the statistics the backward reads
        for _ in range(WARMUP):
            assert call() == 0, lib.toda_last_error()
        us = []
        for _ in range(REPEATS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(CALLS):
                call()
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) / CALLS * 1e3)
        assert lib.toda_device_fault() == 0, lib.toda_last_error()
        result[" ".join(map(str, (op, b, c, hw, f"relu{relu}", f"wide{wide}", "ws" if given else "no-ws")))] = statistics.median(us)
    print("RESULT", json.dumps(result))


def alternate(libs, runs, argv, parse):
    """-> per library the list of its runs' results; children strictly one after another, A first"""
    out = ([], [])
    for i in range(2 * runs):
        p = subprocess.run(argv, env=dict(os.environ, TODA_HIP_LIB=os.path.abspath(libs[i % 2])), capture_output=True, text=True, timeout=900, cwd=ROOT)
        if p.returncode != 0:
            raise SystemExit(f"run {i} ({libs[i % 2]}) ended with {p.returncode}; nothing more is started\n{p.stderr[-3000:]}")
        out[i % 2].append(parse(p.stdout))
    return out


def verdict(name, a, b, unit, higher_is_better=False):
    ma, mb, spread = statistics.median(a), statistics.median(b), max(a) - min(a)
    worse = (ma - mb) if higher_is_better else (mb - ma)
    ok = worse <= spread
    print(f"{name:58s} A {ma:9.2f} (spread {spread:6.2f})  B {mb:9.2f}  B - A {mb - ma:+8.2f} {unit}  {'ok' if ok else 'REGRESSION'}")
    return ok


def kernels(lib_a, lib_b, runs):
    a, b = alternate((lib_a, lib_b), runs, [sys.executable, os.path.abspath(__file__), "child"], lambda out: json.loads(out.split("RESULT")[-1]))
    print(f"A = {lib_a}, B = {lib_b}, {runs} runs of each, alternating; medians in microseconds per call")
    bad = sum(not verdict(k, [r[k] for r in a], [r[k] for r in b], "us") for k in a[0])
    print(f"{len(a[0])} shapes, {bad} where B is slower than A by more than A's own spread")
    return 1 if bad else 0


def steps(lib_a, lib_b, runs):
    argv = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5", "--no-cpu-baseline"]
    a, b = alternate((lib_a, lib_b), runs, argv, lambda out: json.loads(out.strip().splitlines()[-1]))
    a, b = [r["value"] for r in a], [r["value"] for r in b]
    print(f"A = {lib_a}, B = {lib_b}, {runs} runs of each, alternating; bench.py C3 samples/s: A {a}  B {b}")
    return 0 if verdict("bench.py C3", a, b, "samples/s", higher_is_better=True) else 1


if __name__ == "__main__":
    if sys.argv[1:] == ["child"]:
        child()
    elif len(sys.argv) in (4, 5) and sys.argv[1] in ("kernels", "steps"):
        sys.exit((kernels if sys.argv[1] == "kernels" else steps)(sys.argv[2], sys.argv[3], int(sys.argv[4]) if len(sys.argv) == 5 else 3))
    else:
        sys.exit(__doc__)
