"""Observed information and score of a Cox model on an X already on the GPU: cox_information_device against the torch
route.

  python tools/cox_info_bench.py [--repeats 10] [--calls 7] [--p 20000] [--out profiles/cox_info_bench.jsonl]

Writes one JSON line per case.  Cases: the configs[4] shape (n = 200 000, p = 20 000) with a support of m = 150 columns
as fp64 column-major, fp64 row-major and fp32 row-major X; ties="breslow", times on a grid (about a third of the rows
share one), about 70 % events, weights.  Both routes end with the m^2 + m numbers on the host:
  device     capi.cox_information_device(X, cols, beta, time, status, weight, ties="breslow")
  torch      what a user has without it: gather X[:, cols] into an n x m tensor, capi.predict_device for eta, the time
             order from the host, torch flip / cumsum for S0, S1 and H, and two torch.matmul Grams (rocBLAS)
Per case:
  gather_ms, means_ms, launches_ms   bessx_op_cox_info_bench (device events, one warm-up): the gather of e x into
                       position order, the column-wise suffix scan that emits the risk-set means, every launch of a call
  new_kernels_gbps     the bytes the gather and the scan must move / (gather_ms + means_ms);  share_of_copy_rate = that
                       over capi.op_stream_copy_gbps()
  device_s, torch_s    wall time around work that ends with the numbers on the host, the two routes ALTERNATING, --calls
                       each after one warm-up each: median, and min / max as the spread
  torch_over_device    ratio of the medians
  max_rel_diff_of_the_routes   largest |difference| of an entry of the information over sqrt(I_jj I_kk)
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
    ap.add_argument("--out", default=os.path.join("profiles", "cox_info_bench.jsonl"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("cox_info_bench: no GPU (nothing is measured on a CPU)")
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
    # the order, as the host knows it (both routes sort on the host)
    order = np.argsort(tm, kind="stable")
    ts = tm[order]
    new = np.ones(n, dtype=bool)
    new[1:] = ts[1:] != ts[:-1]
    starts = np.nonzero(new)[0]
    first = np.maximum.accumulate(np.where(new, np.arange(n), 0))
    last = np.append(starts[1:] - 1, n - 1)[np.cumsum(new) - 1]
    ev = status[order] != 0
    lines = []
    for name, dt, colmajor in cases:
        g = torch.Generator(device="cuda").manual_seed(1)
        X = torch.randn((p, n) if colmajor else (n, p), generator=g, device="cuda", dtype=dt)
        if colmajor:
            X = X.T
        cols_t = torch.from_numpy(cols.astype(np.int64)).cuda()
        torch.cuda.synchronize()
        (ms0, ms1, ms2), nbytes = capi.op_cox_info_bench(X, cols, ties="breslow", repeats=a.repeats)
        gbps = nbytes / ((ms0 + ms1) * 1e-3) / 1e9
        rec = dict(base, what="cox information", case=name, n=n, p=p, m=m, n_event_rows=J, repeats=a.repeats,
                   gather_ms=ms0, means_ms=ms1, launches_ms=ms2, new_kernels_bytes=nbytes, new_kernels_gbps=gbps,
                   share_of_copy_rate=gbps / copy_gbps, workspace_doubles=capi.cox_info_workspace(n, m, J)[0])

        def device():
            r = capi.cox_information_device(X, cols, beta, tm, status, weight=w, ties="breslow")
            return r["info"], r["score"]

        def torch_route():
            o = torch.from_numpy(order).cuda()
            fi, la = torch.from_numpy(first).cuda(), torch.from_numpy(last).cuda()
            evt = torch.from_numpy(ev).cuda()
            wd = torch.from_numpy((w * status)[order]).cuda()
            Xs = X[:, cols_t].to(torch.float64)[o]
            eta = capi.predict_device(X, cols, beta, [0.0])[o]
            e = torch.exp(torch.clamp(eta, -30.0, 30.0))
            S0 = torch.flip(torch.cumsum(torch.flip(e, [0]), 0), [0])[fi]
            S1 = torch.flip(torch.cumsum(torch.flip(e[:, None] * Xs, [0]), 0), [0])
            H = torch.cumsum(wd / S0, 0)[la]
            v = e * H
            U = S1[fi[evt]] / S0[evt][:, None]
            info = Xs.T @ (Xs * v[:, None]) - U.T @ (U * wd[evt][:, None])
            score = Xs.T @ (wd - v)
            return info.cpu().numpy(), score.cpu().numpy()

        (ia, _), (ib, _) = device(), torch_route()  # warm-up of both, and the two routes must agree
        d = np.sqrt(np.abs(np.diag(ib)))
        rec.update(max_rel_diff_of_the_routes=float(np.max(np.abs(ia - ib) / np.outer(d, d))))
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
