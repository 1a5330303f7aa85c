"""Held-out Cox partial likelihood and concordance on an X already on the GPU, against the route a user has without it.

  python tools/cox_eval_bench.py [--n 200000 --p 2000] [--m 150] [--repeats 5] [--calls 5] [--no-baseline-pairs]
                                 [--out profiles/cox_eval_bench.jsonl]

Writes one JSON line per case.  The design has the rows of configs[4] (n = 200 000) and fewer columns, fp64 row-major,
made on the device; the support is m = 150 columns drawn at random; R = 1 model and the R = 150 candidates of a path
(candidate r uses the first r + 1 columns of the support).  Times are distinct, about half the rows are events.
Both routes end with the numbers on the host:
  device     capi.evaluate_cox_device(X, cols, B, time, status), with and without concordance
  baseline   capi.predict_device with the identity link, the n x R predictions copied to the host, then the NumPy route
             of bess_base.evaluate_survival (linear.bess_base._survival_host) per model.  Its O(n^2) pair counts take
             minutes per model at this n: they are timed for R = 1 only, ONE call (--no-baseline-pairs leaves them out);
             the likelihood alone is timed for both R
Per case:
  stage_ms                     bessx_op_cox_eval_bench (device events, one warm-up launch per stage): predictor pass,
                               risk-set scan + likelihood reduction, pair counts
  device_s, device_nopairs_s   wall time (host clock around work that ends with the numbers on the host), the device
  baseline_loglik_s            routes and the baseline likelihood ALTERNATING, --calls each after one warm-up each:
                               median, min and max as the spread
  baseline_pairs_s             R = 1: the baseline with its pair counts, one call
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bess_amd import capi, linear  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--p", type=int, default=2000)
    ap.add_argument("--m", type=int, default=150)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--no-baseline-pairs", action="store_true")
    ap.add_argument("--label", default="this build")
    ap.add_argument("--out", default=os.path.join("profiles", "cox_eval_bench.jsonl"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("cox_eval_bench: no GPU (nothing is measured on a CPU)")
    n, p, m = a.n, a.p, a.m
    g = torch.Generator(device="cuda").manual_seed(1)
    X = torch.randn((n, p), generator=g, device="cuda", dtype=torch.float64)
    torch.cuda.synchronize()
    rng = np.random.default_rng(3)
    cols = np.sort(rng.choice(p, m, replace=False)).astype(np.int32)
    tm = rng.permutation(n).astype(np.float64)
    status = (rng.uniform(size=n) < 0.5).astype(np.float64)
    ones = np.ones(n)
    base = {"device": capi.device_info(), "n": n, "p": p, "m": m, "source": "fp64 row-major", "label": a.label}
    lines = []
    for R in (1, m):
        B = np.zeros((m, R))
        for r in range(R):
            k = m if R == 1 else r + 1
            B[:k, r] = rng.standard_normal(k) / np.sqrt(k)
        rec = dict(base, what="cox_evaluate", R=R, repeats=a.repeats, calls=a.calls)
        rec["stage_ms"] = list(capi.op_cox_eval_bench(X, cols, R=R, repeats=a.repeats))

        def device():
            return capi.evaluate_cox_device(X, cols, B, tm, status)

        def device_nopairs():
            return capi.evaluate_cox_device(X, cols, B, tm, status, concordance=False)

        def baseline(pairs=False):
            eta = capi.predict_device(X, cols, B, np.zeros(R)).cpu().numpy()
            return [linear.bess_base._survival_host(np.ascontiguousarray(eta[:, r]), tm, status, ones, "order", pairs)
                    for r in range(R)]

        legs = {"device": device, "device_nopairs": device_nopairs, "baseline_loglik": baseline}
        warm = {k: fn() for k, fn in legs.items()}
        ll_b = np.array([v[0] for v in warm["baseline_loglik"]])
        rec["max_rel_diff_of_the_routes"] = float(np.max(np.abs(warm["device"]["loglik"] - ll_b) / np.abs(ll_b)))
        times = {k: [] for k in legs}
        for _ in range(a.calls):
            for k, fn in legs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[k].append(time.perf_counter() - t0)
        for k, v in times.items():
            rec.update({k + "_s": statistics.median(v), k + "_min_s": min(v), k + "_max_s": max(v)})
        rec["baseline_loglik_over_device_nopairs"] = rec["baseline_loglik_s"] / rec["device_nopairs_s"]
        rec["pairs_share_of_device_s"] = 1.0 - rec["device_nopairs_s"] / rec["device_s"]
        if R == 1 and not a.no_baseline_pairs:
            t0 = time.perf_counter()
            got = baseline(True)[0]
            rec["baseline_pairs_s"] = time.perf_counter() - t0
            rec["baseline_pairs_over_device"] = rec["baseline_pairs_s"] / rec["device_s"]
            d = warm["device"]
            rec["counts_equal"] = bool((got[1], got[2], got[3]) == (d["comparable"], int(d["concordant"][0]),
                                                                    int(d["discordant"][0])))
        lines.append(rec)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
            print(json.dumps(ln), flush=True)


if __name__ == "__main__":
    main()
