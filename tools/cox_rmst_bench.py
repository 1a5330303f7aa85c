"""Restricted mean and quantile survival times of a Cox model on an X already on the GPU, against the route a user has
without them.

  python tools/cox_rmst_bench.py [--n 200000 --p 2000] [--m 150] [--T 1 100] [--Q 5] [--small-n 1000] [--repeats 3]
                                 [--calls 7] [--block-mb 512] [--step-timeout 300] [--out profiles/cox_rmst_bench.jsonl]

The parent process only starts one child per case (layout of X x T), each under its own time limit, and stops at the
first child that fails; a child makes the design on the device (the rows of configs[4], n = 200 000, fewer columns), draws
m = 150 support columns, fits the baseline on these rows (about 70 % events at distinct times: J about 140 000), measures,
and appends one JSON line to --out.  Layouts of X: fp64 row-major, fp64 column-major, fp32 row-major; one more case runs
the first --small-n rows of the fp64 row-major design against the same baseline, to show whether the split of the
segments over workgroups fills the device when the rows alone would not.
Per case:
  stage_ms             bessx_op_cox_rmst_bench (device events, one warm-up launch per stage) for K = J + T segments: the
                       predictor pass that stores exp(clip(eta)), k_cxr_partial, k_cxr_finish, k_cxr_quantile
  partial_gterms_s     n * K terms of exp per second of k_cxr_partial / 1e9 (k_cxs_curves writes 403 - 428 G elements/s of
                       the same exp with a store per element)
  fused_s, torch_s     wall time (host clock around work that ends in a device synchronise) of
                       capi.cox_survival_times_device (T horizons and Q levels in one call) and of the route it replaces:
                       capi.predict_device + exp, then per block of segments torch.exp(-(e[:, None] * hs[None, :])) @ wd
                       (--block-mb: the size of that n x block matrix) and torch.searchsorted for the quantiles,
                       ALTERNATING, --calls each after one warm-up each: median, min and max as the spread
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


def child(a, layout, T, rows):
    import torch
    from bess_amd import capi
    if not torch.cuda.is_available():
        raise SystemExit("cox_rmst_bench: no GPU (nothing is measured on a CPU)")
    n, p, m, Q = a.n, a.p, a.m, a.Q
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
    tm = rng.permutation(n).astype(np.float64) + 1.0
    status = (rng.uniform(size=n) < 0.7).astype(np.float64)
    zero = np.zeros(1)
    base = capi.cox_baseline_device(X, cols, B, tm, status)
    bt, bh = base["times"], base["cumhaz"]
    if rows < n:
        X, n = X[:rows], rows
    tau = np.quantile(bt, (np.arange(T) + 1.0) / T)  # the last horizon is the last event time: every segment is used
    q = (np.arange(Q) + 1.0) / (Q + 1.0)
    hs, wd, cut = capi.rmst_segments(bt, bh, tau)
    K, J = int(hs.size), int(bt.size)
    rec = {"device": capi.device_info(), "what": "cox_rmst", "n": n, "p": p, "m": m, "T": T, "Q": Q, "J": J, "K": K,
           "source": layout, "label": a.label, "repeats": a.repeats, "calls": a.calls, "block_mb": a.block_mb,
           "workspace": capi.cox_survtime_workspace(n, cut)}
    rec["stage_ms"] = list(capi.op_cox_rmst_bench(X, cols, K=K, T=T, J=J, Q=Q, repeats=a.repeats))
    rec["partial_gterms_s"] = n * float(K) / (rec["stage_ms"][1] * 1e-3) / 1e9
    hs_d, wd_d = torch.from_numpy(hs).cuda(), torch.from_numpy(wd).cuda()
    hz_d, ut_d = torch.from_numpy(bh).cuda(), torch.from_numpy(np.append(bt, np.inf)).cuda()
    c_d = torch.from_numpy(capi.survival_levels(q)).cuda()
    order = np.argsort(cut, kind="stable")
    block = max(1, (a.block_mb << 20) // (8 * n))

    def fused():
        return capi.cox_survival_times_device(X, cols, B, bt, bh, tau=tau, q=q)

    def torch_route():
        e = torch.exp(torch.clamp(capi.predict_device(X, cols, B, zero).reshape(-1), -30.0, 30.0))
        out = torch.empty((n, T), dtype=torch.float64, device="cuda")
        acc = torch.zeros(n, dtype=torch.float64, device="cuda")
        k = 0
        for j in order:
            while k < cut[j]:
                kk = min(int(cut[j]), k + block)
                acc = acc + torch.exp(-(e[:, None] * hs_d[None, k:kk])) @ wd_d[k:kk]
                k = kk
            out[:, j] = acc
        idx = torch.searchsorted(hz_d, (c_d[None, :] / e[:, None]).contiguous())  # (the level over e, not the product)
        return {"rmst": out, "quantile": ut_d[idx]}

    want, got = torch_route(), fused()
    rec["max_rel_diff_of_the_rmst_routes"] = float(((want["rmst"] - got["rmst"]).abs() / want["rmst"]).max())
    rec["quantiles_that_differ"] = int((want["quantile"] != got["quantile"]).sum())
    del want, got
    rec.update(_alternate({"fused": fused, "torch": torch_route}, a.calls, torch.cuda.synchronize))
    rec["torch_over_fused"] = rec["torch_s"] / rec["fused_s"]
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
    ap.add_argument("--Q", type=int, default=5)
    ap.add_argument("--small-n", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--block-mb", type=int, default=512)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--label", default="this build")
    ap.add_argument("--out", default=os.path.join("profiles", "cox_rmst_bench.jsonl"))
    ap.add_argument("--case", nargs=3, metavar=("LAYOUT", "T", "ROWS"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.case:
        child(a, a.case[0], int(a.case[1]), int(a.case[2]))
        return
    passed = [x for x in sys.argv[1:]]
    cases = [(layout, T, a.n) for layout in LAYOUTS for T in a.T]
    if 0 < a.small_n < a.n:
        cases += [(LAYOUTS[0], T, a.small_n) for T in a.T]
    for layout, T, rows in cases:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__)] + passed + [
            "--case", layout, str(T), str(rows)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:  # (a step that failed, faulted or ran out of time: nothing more is started on the GPU)
            raise SystemExit("cox_rmst_bench: %s, T = %d, %d rows ended with status %d" % (layout, T, rows, rc))


if __name__ == "__main__":
    main()
