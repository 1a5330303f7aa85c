"""Baseline hazard and survival curves of a Cox model on an X already on the GPU, against the routes a user has without
them.

  python tools/cox_surv_bench.py [--n 200000 --p 2000] [--m 150] [--T 1 100] [--repeats 5] [--calls 5]
                                 [--step-timeout 300] [--out profiles/cox_surv_bench.jsonl]

The parent process only starts one child per case (layout of X x T), each under its own time limit, and stops at the
first child that fails; a child makes the design on the device (the rows of configs[4], n = 200 000, fewer columns), draws
m = 150 support columns, measures, and appends one JSON line to --out.  Layouts of X: fp64 row-major, fp64 column-major,
fp32 row-major.  Times are distinct, about half the rows are events.
Per case:
  stage_ms               bessx_op_cox_surv_bench (device events, one warm-up launch per stage): the predictor pass that
                         stores exp(clip(eta)) in row order, k_cxs_curves (row-major result), the baseline's hazard terms +
                         forward scan + gather; stage_ms_col_major: the same for a column-major result
  copy_gbps              bessx_op_stream_copy_gbps (read + write bytes / time) in the same process
  curves_share_of_copy   n * T * 8 bytes written / the time of k_cxs_curves, as a fraction of copy_gbps
  curves_s, torch_s      wall time (host clock around work that ends in a device synchronise) of capi.cox_survival_device
                         and of the route it replaces, capi.predict_device + exp(-exp(clamp(eta))[:, None] * Hg[None, :])
                         in torch, ALTERNATING, --calls each after one warm-up each: median, min and max as the spread
  baseline_s, numpy_s    (T = the first of --T only) capi.cox_baseline_device against capi.predict_device + copy to the
                         host + the NumPy route (linear.bess_base._baseline_host), the same way
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LAYOUTS = ("fp64 row-major", "fp64 column-major", "fp32 row-major")


def _alternate(legs, calls, sync):
    for fn in legs.values():  # one warm-up each
        fn()
    times = {k: [] for k in legs}
    for _ in range(calls):
        for k, fn in legs.items():
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            times[k].append(time.perf_counter() - t0)
    out = {}
    for k, v in times.items():
        out.update({k + "_s": statistics.median(v), k + "_min_s": min(v), k + "_max_s": max(v)})
    return out


def child(a, layout, T, with_baseline):
    import torch
    from bess_amd import capi, linear
    if not torch.cuda.is_available():
        raise SystemExit("cox_surv_bench: no GPU (nothing is measured on a CPU)")
    n, p, m = a.n, a.p, a.m
    g = torch.Generator(device="cuda").manual_seed(1)
    dtype = torch.float32 if layout.startswith("fp32") else torch.float64
    if layout.endswith("column-major"):
        X = torch.randn((p, n), generator=g, device="cuda", dtype=dtype).T
    else:
        X = torch.randn((n, p), generator=g, device="cuda", dtype=dtype)
    torch.cuda.synchronize()
    rng = np.random.default_rng(3)
    cols = np.sort(rng.choice(p, m, replace=False)).astype(np.int32)
    B = rng.standard_normal(m) / np.sqrt(m)
    tm = rng.permutation(n).astype(np.float64)
    status = (rng.uniform(size=n) < 0.5).astype(np.float64)
    ones, zero = np.ones(n), np.zeros(1)
    rec = {"device": capi.device_info(), "what": "cox_survival", "n": n, "p": p, "m": m, "T": T, "source": layout,
           "label": a.label, "repeats": a.repeats, "calls": a.calls}
    rec["stage_ms"] = list(capi.op_cox_surv_bench(X, cols, T=T, repeats=a.repeats))
    rec["stage_ms_col_major"] = list(capi.op_cox_surv_bench(X, cols, T=T, out_col_major=True, repeats=a.repeats))
    rec["copy_gbps"] = capi.op_stream_copy_gbps(1 << 28, 20)
    for key, ms in (("curves_share_of_copy", rec["stage_ms"][1]),
                    ("curves_col_major_share_of_copy", rec["stage_ms_col_major"][1])):
        rec[key] = (n * T * 8.0 / (ms * 1e-3) / 1e9) / rec["copy_gbps"]
    base = capi.cox_baseline_device(X, cols, B, tm, status)
    grid = np.quantile(base["times"], (np.arange(T) + 0.5) / T)
    hg_dev = torch.from_numpy(capi.baseline_at(base["times"], base["cumhaz"], grid)).cuda()

    def curves():
        return capi.cox_survival_device(X, cols, B, base["times"], base["cumhaz"], times=grid)

    def torch_route():
        eta = capi.predict_device(X, cols, B, zero)
        return torch.exp(-torch.exp(torch.clamp(eta, -30.0, 30.0))[:, None] * hg_dev[None, :])

    want, got = torch_route(), curves()
    rec["max_abs_diff_of_the_curve_routes"] = float((want - got).abs().max())
    del want, got
    rec.update(_alternate({"curves": curves, "torch": torch_route}, a.calls, torch.cuda.synchronize))
    rec["torch_over_curves"] = rec["torch_s"] / rec["curves_s"]
    if with_baseline:
        def baseline():
            return capi.cox_baseline_device(X, cols, B, tm, status)

        def numpy_route():
            eta = capi.predict_device(X, cols, B, zero).cpu().numpy()
            return linear.bess_base._baseline_host(eta, tm, status, ones)

        h = numpy_route()[1]
        rec["max_rel_diff_of_the_baseline_routes"] = float(np.max(np.abs(base["cumhaz"] - h) / h))
        rec.update(_alternate({"baseline": baseline, "numpy": numpy_route}, a.calls, torch.cuda.synchronize))
        rec["numpy_over_baseline"] = rec["numpy_s"] / rec["baseline_s"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--p", type=int, default=2000)
    ap.add_argument("--m", type=int, default=150)
    ap.add_argument("--T", type=int, nargs="+", default=[1, 100])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--label", default="this build")
    ap.add_argument("--out", default=os.path.join("profiles", "cox_surv_bench.jsonl"))
    ap.add_argument("--case", nargs=3, metavar=("LAYOUT", "T", "BASELINE"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.case:
        child(a, a.case[0], int(a.case[1]), a.case[2] == "1")
        return
    passed = [x for x in sys.argv[1:]]
    for layout in LAYOUTS:
        for T in a.T:
            cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__)] + passed + [
                "--case", layout, str(T), "1" if T == a.T[0] else "0"]
            rc = subprocess.run(cmd).returncode
            if rc != 0:  # (a step that failed, faulted or ran out of time: nothing more is started on the GPU)
                raise SystemExit("cox_surv_bench: %s, T = %d ended with status %d" % (layout, T, rc))


if __name__ == "__main__":
    main()
