"""Residuals, dfbeta and case influence of a Cox model on an X already on the GPU: cox_diagnostics_device against the
torch route.

  python tools/cox_diag_bench.py [--repeats 10] [--calls 7] [--p 20000] [--out profiles/cox_diag_bench.jsonl]

Writes one JSON line per case.  Cases: the configs[4] shape (n = 200 000, p = 20 000) with a support of m = 150 columns
as fp64 column-major, fp64 row-major and fp32 row-major X; ties="breslow", times on a grid (about a third of the rows
share one), about 70 % events, weights; a ready factor R and C = R^T R from cox_information_device + info_factor.  Both
routes end with every kind (martingale, deviance, score, dfbeta, displacement, schoenfeld) as tensors on the device:
  device     capi.cox_diagnostics_device(X, cols, beta, time, status, factor=R, cinv=C, weight, ties="breslow")
  torch      what a user has without it: gather X[:, cols] into an n x m tensor, capi.predict_device for eta, the time
             order from the host, torch flip / cumsum for S0 and S1, cumsum for H and A, and L @ C (rocBLAS)
Per case:
  accum_ms, form_ms, displacement_ms, dfbeta_ms   bessx_op_cox_diag_bench (device events, one warm-up): the increments and
                       their forward scan, those plus the forming of L, L R^T with the displacement epilogue, L C with the
                       dfbeta epilogue
  apply_tflops         fp64 TFLOP/s of the dfbeta launch over 2 n Mpad^2 operations, Mpad = 16 ceil(m / 16)
  device_s, torch_s    wall time around work that ends with the tensors on the device, the two routes ALTERNATING, --calls
                       each after one warm-up each: median, and min / max as the spread
  torch_over_device    ratio of the medians (below 1: the device route is slower)
  max_rel_diff_of_the_routes   largest |difference| of a dfbeta entry over the largest |dfbeta| of its column
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
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--p", type=int, default=20000)
    ap.add_argument("--m", type=int, default=150)
    ap.add_argument("--label", default="this build")
    ap.add_argument("--out", default=os.path.join("profiles", "cox_diag_bench.jsonl"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("cox_diag_bench: no GPU (nothing is measured on a CPU)")
    n, p, m = a.n, a.p, a.m
    cases = [("configs[4] fp64 column-major", torch.float64, True), ("configs[4] fp64 row-major", torch.float64, False),
             ("configs[4] fp32 row-major", torch.float32, False)]
    base = {"device": capi.device_info(), "label": a.label}
    rng = np.random.default_rng(3)
    cols = np.sort(rng.choice(p, m, replace=False)).astype(np.int32)
    beta = rng.standard_normal(m) / np.sqrt(m)
    tm = rng.integers(0, int(2.5 * n) + 1, n) / 8.0
    status = (rng.uniform(size=n) < 0.7).astype(np.float64)
    w = rng.integers(1, 17, n) / 8.0
    J = int(status.sum())
    # the order, as the host knows it (both routes sort on the host)
    order = np.argsort(tm, kind="stable")
    ts = tm[order]
    new = np.ones(n, dtype=bool)
    new[1:] = ts[1:] != ts[:-1]
    starts = np.nonzero(new)[0]
    first = np.maximum.accumulate(np.where(new, np.arange(n), 0))
    last = np.append(starts[1:] - 1, n - 1)[np.cumsum(new) - 1]
    ev = status[order] != 0
    inv = np.empty(n, dtype=np.int64)
    inv[order] = np.arange(n)
    mpad = 16 * ((m + 15) // 16)
    lines = []
    for name, dt, colmajor in cases:
        g = torch.Generator(device="cuda").manual_seed(1)
        X = torch.randn((p, n) if colmajor else (n, p), generator=g, device="cuda", dtype=dt)
        if colmajor:
            X = X.T
        cols_t = torch.from_numpy(cols.astype(np.int64)).cuda()
        torch.cuda.synchronize()
        info = capi.cox_information_device(X, cols, beta, tm, status, weight=w, ties="breslow")["info"]
        R, pd = capi.info_factor(info)
        if not pd:
            raise SystemExit("cox_diag_bench: the information matrix is not positive definite")
        C = R.T @ R
        (ms0, ms1, ms2, ms3), nbytes = capi.op_cox_diag_bench(X, cols, ties="breslow", repeats=a.repeats)
        rec = dict(base, what="cox diagnostics", case=name, n=n, p=p, m=m, n_event_rows=J, repeats=a.repeats,
                   accum_ms=ms0, form_ms=ms1, displacement_ms=ms2, dfbeta_ms=ms3, kernels_bytes=nbytes,
                   apply_tflops=2.0 * n * mpad * mpad / (ms3 * 1e-3) / 1e12,
                   workspace_doubles=capi.cox_diag_workspace(n, m, J))

        def device():
            return capi.cox_diagnostics_device(X, cols, beta, tm, status, factor=R, cinv=C, weight=w, ties="breslow")

        def torch_route():
            o, back = torch.from_numpy(order).cuda(), torch.from_numpy(inv).cuda()
            fi, la = torch.from_numpy(first).cuda(), torch.from_numpy(last).cuda()
            evt = torch.from_numpy(ev).cuda()
            wd = torch.from_numpy((w * status)[order]).cuda()
            Ct, Rt = torch.from_numpy(C).cuda(), torch.from_numpy(R).cuda()
            Xs = X[:, cols_t].to(torch.float64)[o]
            eta = capi.predict_device(X, cols, beta, [0.0])[o]
            e = torch.exp(torch.clamp(eta, -30.0, 30.0))
            S0 = torch.flip(torch.cumsum(torch.flip(e, [0]), 0), [0])[fi]
            u = torch.flip(torch.cumsum(torch.flip(e[:, None] * Xs, [0]), 0), [0])[fi] / S0[:, None]
            h = wd / S0
            v = e * torch.cumsum(h, 0)[la]
            gm = wd - v
            A = torch.cumsum(h[:, None] * u, 0)[la]
            L = gm[:, None] * Xs - wd[:, None] * u + e[:, None] * A
            dd = (v - wd) + torch.where(wd == 0, torch.zeros_like(wd), wd * torch.log(torch.where(wd == 0, v, wd) / v))
            T = L @ Rt.T
            return {"martingale": gm[back], "deviance": (torch.sign(gm) * torch.sqrt(2.0 * torch.clamp(dd, min=0.0)))[back],
                    "score": L[back], "dfbeta": (L @ Ct)[back], "displacement": (T * T).sum(1)[back],
                    "schoenfeld": Xs[evt] - u[evt]}

        ra, rb = device(), torch_route()  # warm-up of both, and the two routes must agree
        da, db = ra["dfbeta"].cpu().numpy(), rb["dfbeta"].cpu().numpy()
        rec.update(max_rel_diff_of_the_routes=float(np.max(np.abs(da - db) / np.abs(db).max(axis=0))))
        del ra, rb, da, db
        times = {"device": [], "torch": []}
        for _ in range(a.calls):
            for leg, fn in (("device", device), ("torch", torch_route)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[leg].append(time.perf_counter() - t0)
        md, mt = statistics.median(times["device"]), statistics.median(times["torch"])
        rec.update(device_s=md, device_min_s=min(times["device"]), device_max_s=max(times["device"]), torch_s=mt,
                   torch_min_s=min(times["torch"]), torch_max_s=max(times["torch"]), calls=a.calls,
                   torch_over_device=mt / md)
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
