"""The proportional-hazards test of a Cox model on an X already on the GPU: the three-weight Gram sweep of
cox_zph_device against three one-weight sweeps of the information kernels, and the whole call against
cox_information_device.

  python tools/cox_zph_bench.py [--repeats 15] [--calls 5] [--p 20000] [--out profiles/cox_zph_bench.jsonl]

Shape: configs[4] of bench.py (n = 200 000, p = 20 000), a support of 150 columns, as fp64 column-major, fp64 row-major
and fp32 row-major.  Per case one JSON line:
  fused_ms, separate_ms        bessx_op_cox_zph_bench (device events, one warm-up of each, then `repeats` single timings
                               of each, alternating): ONE launch of k_cxz_gram with its finish for three row-weight pairs
                               against THREE back-to-back launch_info_gram sweeps on the same data; medians, with min and
                               max as the spread
  separate_over_fused          the ratio of the medians = the fused sweep's matrix-core rate as a multiple of the
                               existing sweep's (both do the same 3 * 2 n (m + 1) (m + 2) operations)
  fused_tflops, separate_tflops, fused_support_gbps (the support's n m elements once) and its share of the device copy rate
  fused_wins                   the fused median is below the separate one by more than the larger of the two spreads
  zph_s, info_s                wall time of cox_zph_device and of cox_information_device, results on the host (medians of
                               `calls`, min / max): what the three matrices cost on top of the one
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bess_amd import capi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--p", type=int, default=20000)
    ap.add_argument("--m", type=int, default=150)
    ap.add_argument("--label", default="this build")
    ap.add_argument("--out", default=os.path.join("profiles", "cox_zph_bench.jsonl"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("cox_zph_bench: no GPU (nothing is measured on a CPU)")
    n, p, m = a.n, a.p, a.m
    cases = [("configs[4] fp64 column-major", torch.float64, True), ("configs[4] fp64 row-major", torch.float64, False),
             ("configs[4] fp32 row-major", torch.float32, False)]
    copy_gbps = capi.op_stream_copy_gbps()
    base = {"device": capi.device_info(), "label": a.label, "copy_gbps": copy_gbps}
    rng = np.random.default_rng(3)
    cols = np.sort(rng.choice(p, m, replace=False)).astype(np.int32)
    beta = rng.standard_normal(m) / np.sqrt(m)
    tm = rng.integers(0, int(2.5 * n) + 1, n) / 8.0
    status = (rng.uniform(size=n) < 0.7).astype(np.float64)
    w = rng.integers(1, 17, n) / 8.0
    J = int(status.sum())
    gt = capi.zph_transform(tm, status, w, "km")[0]
    flops = 3 * 2.0 * n * (m + 1) * (m + 2)
    lines = []
    for name, dt, colmajor in cases:
        g = torch.Generator(device="cuda").manual_seed(1)
        X = torch.randn((p, n) if colmajor else (n, p), generator=g, device="cuda", dtype=dt)
        if colmajor:
            X = X.T
        torch.cuda.synchronize()
        fused, sep = capi.op_cox_zph_bench(X, cols, repeats=a.repeats)
        mf, ms = statistics.median(fused), statistics.median(sep)
        spread = max(fused.max() - fused.min(), sep.max() - sep.min())
        gbps = n * m * X.element_size() / (mf * 1e-3) / 1e9
        rec = dict(base, what="cox zph", case=name, n=n, p=p, m=m, n_event_rows=J, repeats=a.repeats,
                   fused_ms=mf, fused_min_ms=float(fused.min()), fused_max_ms=float(fused.max()),
                   separate_ms=ms, separate_min_ms=float(sep.min()), separate_max_ms=float(sep.max()),
                   separate_over_fused=ms / mf, fused_tflops=flops / (mf * 1e-3) / 1e12,
                   separate_tflops=flops / (ms * 1e-3) / 1e12, fused_support_gbps=gbps,
                   fused_share_of_copy_rate=gbps / copy_gbps, fused_wins=bool(ms - mf > spread),
                   workspace_doubles=capi.cox_zph_workspace(n, m, J)[0])
        legs = {"zph": lambda: capi.cox_zph_device(X, cols, beta, tm, status, gt, weight=w, ties="breslow"),
                "info": lambda: capi.cox_information_device(X, cols, beta, tm, status, weight=w, ties="breslow")}
        times = {k: [] for k in legs}
        for i in range(-1, a.calls):  # (i = -1: the warm-up of both)
            for leg, fn in legs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if i >= 0:
                    times[leg].append(time.perf_counter() - t0)
        for leg, ts in times.items():
            rec.update({leg + "_s": statistics.median(ts), leg + "_min_s": min(ts), leg + "_max_s": max(ts)})
        rec.update(calls=a.calls, zph_over_info=rec["zph_s"] / rec["info_s"])
        lines.append(rec)
        print(json.dumps(rec), flush=True)
        del X
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
