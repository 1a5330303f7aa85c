"""The IPCW Brier score of the candidates of a Cox path on an X already on the GPU: the fused reduction against the route a
user has without it.

  python tools/cox_brier_bench.py [--n 200000 --p 2000] [--m 150] [--T 100] [--R 1 150] [--repeats 5] [--calls 7]
                                  [--step-timeout 600] [--out profiles/cox_brier_bench.jsonl]

The parent process only starts one child per case (layout of X x R), each under its own time limit, and stops at the
first child that fails; a child makes the design on the device (the validation rows of configs[4], n = 200 000, fewer
columns), draws m = 150 support columns, gives candidate r the first m - R + r + 1 of them (a path: nested supports, the
last one full), measures, and appends one JSON line to --out.  Layouts of X: fp64 column-major, fp64 row-major, fp32
row-major.  Times are distinct, about 60% of the rows are events, the T requested times are quantiles of the row times,
the weights are Kaplan-Meier (capi.ipcw_weights).
Per case:
  stage_ms               bessx_op_cox_brier_bench (device events, one warm-up launch per stage): the predictor pass that
                         stores exp(clip(eta)) as R x n, the reduction kernel k_cxb_terms, the addition of its slabs
  terms_gelem_s          n * T * R elements / the time of k_cxb_terms: one transcendental, a compare, a square and a
                         multiply-add each, nothing stored
  curves_gelem_s         n * T elements / the time of k_cxs_curves (bessx_op_cox_surv_bench, row-major result) at the same
                         n and T: the same exp per element, and the element is written
  fused_s, torch_s       wall time (host clock around work that ends in a device synchronise) of ONE capi.cox_brier_device
                         call for the R models and of the route it replaces -- per model capi.predict_device on the model's
                         own support, then the n x T matrix S = exp(-e hg) and the weighted sums in torch -- ALTERNATING,
                         --calls each after one warm-up each: median, min and max as the spread.  Both routes form the
                         IPCW weights on the host (capi.ipcw_weights) and upload the row vectors inside the timed call;
                         the fused call also returns the null model, IPA and the integrals, the torch route only BS.
  max_rel_diff           of the two routes' scores
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
LAYOUTS = ("fp64 column-major", "fp64 row-major", "fp32 row-major")


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


def child(a, layout, R):
    import torch
    from bess_amd import capi
    if not torch.cuda.is_available():
        raise SystemExit("cox_brier_bench: no GPU (nothing is measured on a CPU)")
    n, p, m, T = a.n, a.p, a.m, a.T
    g = torch.Generator(device="cuda").manual_seed(1)
    dtype = torch.float32 if layout.startswith("fp32") else torch.float64
    if layout.endswith("column-major"):
        X = torch.randn((p, n), generator=g, device="cuda", dtype=dtype).T
    else:
        X = torch.randn((n, p), generator=g, device="cuda", dtype=dtype)
    torch.cuda.synchronize()
    rng = np.random.default_rng(3)
    cols = np.sort(rng.choice(p, m, replace=False)).astype(np.int32)
    B = np.zeros((m, R))
    for r in range(R):
        k = m - R + r + 1
        B[:k, r] = rng.standard_normal(k) / np.sqrt(k)
    tm = rng.permutation(n).astype(np.float64) + 1.0
    status = (rng.uniform(size=n) < 0.6).astype(np.float64)
    times = np.quantile(tm, (np.arange(T) + 0.5) / T * 0.8)
    hg = np.outer((np.arange(T) + 1.0) / T, 1.0 + np.arange(R) / R)
    zero = np.zeros(1)
    rec = {"device": capi.device_info(), "what": "cox_brier", "n": n, "p": p, "m": m, "T": T, "R": R, "source": layout,
           "label": a.label, "repeats": a.repeats, "calls": a.calls, "workspace_doubles": capi.cox_brier_workspace(n, T, R)[0]}
    rec["stage_ms"] = list(capi.op_cox_brier_bench(X, cols, R=R, T=T, repeats=a.repeats))
    rec["terms_gelem_s"] = n * T * R / (rec["stage_ms"][1] * 1e-3) / 1e9
    rec["curves_ms"] = capi.op_cox_surv_bench(X, cols, T=T, repeats=a.repeats)[1]
    rec["curves_gelem_s"] = n * T / (rec["curves_ms"] * 1e-3) / 1e9
    d = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()

    def fused():
        return capi.cox_brier_device(X, cols, B, hg, times, tm, status)["brier"]

    def torch_route():
        row_a, time_b = capi.ipcw_weights(tm, status, times)  # (both routes form the weights on the host, per call)
        tm_d, wa_d, b_d, hg_d, t_d = d(tm), d(row_a), d(time_b), d(hg), d(times)
        left = tm_d[:, None] <= t_d[None, :]
        out = torch.empty((T, R), dtype=torch.float64, device="cuda")
        for r in range(R):
            k = m - R + r + 1
            eta = capi.predict_device(X, cols[:k], B[:k, r], zero)
            nz = -(torch.exp(torch.clamp(eta, -30.0, 30.0))[:, None] * hg_d[None, :, r])  # the n x T matrix of one model
            s = torch.exp(nz)
            q = torch.expm1(nz)
            out[:, r] = (torch.where(left, wa_d[:, None] * (s * s), b_d[None, :] * (q * q))).sum(dim=0) / n
        return out.cpu().numpy()

    want, got = torch_route(), fused()
    rec["max_rel_diff"] = float(np.max(np.abs(want - got) / np.maximum(np.abs(want), 1e-300)))
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
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--R", type=int, nargs="+", default=[1, 150])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--step-timeout", type=int, default=600)
    ap.add_argument("--label", default="this build")
    ap.add_argument("--out", default=os.path.join("profiles", "cox_brier_bench.jsonl"))
    ap.add_argument("--case", nargs=2, metavar=("LAYOUT", "R"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.case:
        child(a, a.case[0], int(a.case[1]))
        return
    if max(a.R) > a.m:
        raise SystemExit("cox_brier_bench: R must be at most m (nested supports)")
    passed = [x for x in sys.argv[1:]]
    for layout in LAYOUTS:
        for R in a.R:
            cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__)] + passed + [
                "--case", layout, str(R)]
            rc = subprocess.run(cmd).returncode
            if rc != 0:  # (a step that failed, faulted or ran out of time: nothing more is started on the GPU)
                raise SystemExit("cox_brier_bench: %s, R = %d ended with status %d" % (layout, R, rc))


if __name__ == "__main__":
    main()
