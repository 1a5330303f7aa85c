"""Information matrix and score of one model on an X already on the GPU: information_device against the torch route.

  python tools/info_bench.py [--repeats 20] [--calls 9] [--out profiles/info_bench.jsonl]

Writes one JSON line per case.  Cases: the configs[1] shape (n = 50 000, p = 10 000) with a support of m = 200 columns as
fp64 row-major, fp64 column-major and fp32 row-major X; the configs[2] shape (n = 100 000, p = 5 000) with m = 100, fp64
row-major.  Logistic link, weights.  Both routes end with the (m + 1)^2 + (m + 1) numbers on the host:
  device     capi.information_device(X, cols, beta, coef0, y_dev, link="logistic", weight=w_dev)
  torch      what a user has without it: gather X[:, cols] into an n x m tensor, capi.predict_device for eta, the
             working weights in torch, an n x (m + 1) scaled copy, and one matrix product (rocBLAS) each for the
             information and the score
Per case:
  gram_ms              bessx_op_info_bench (device events, one warm-up: k_info_gram + k_info_finish alone)
  gram_tflops          2 n (m + 1) (m + 2) operations / gram_ms;  share_of_fp64_matrix_peak = gram_tflops / 78.6
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

PEAK_FP64_MATRIX_TFLOPS = 78.6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--label", default="this build")
    ap.add_argument("--out", default=os.path.join("profiles", "info_bench.jsonl"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("info_bench: no GPU (nothing is measured on a CPU)")
    cases = [("configs[1] fp64 row-major", 50000, 10000, 200, torch.float64, False),
             ("configs[1] fp64 column-major", 50000, 10000, 200, torch.float64, True),
             ("configs[1] fp32 row-major", 50000, 10000, 200, torch.float32, False),
             ("configs[2] fp64 row-major", 100000, 5000, 100, torch.float64, False)]
    base = {"device": capi.device_info(), "label": a.label}
    lines = []
    for name, n, p, m, dt, colmajor in cases:
        g = torch.Generator(device="cuda").manual_seed(1)
        X = torch.randn((n, p), generator=g, device="cuda", dtype=dt)
        if colmajor:
            X = X.T.contiguous().T
        y = (torch.rand((n,), generator=g, device="cuda", dtype=torch.float64) < 0.5).to(torch.float64)
        w = torch.rand((n,), generator=g, device="cuda", dtype=torch.float64) + 0.5
        rng = np.random.default_rng(3)
        cols = np.sort(rng.choice(p, m, replace=False)).astype(np.int32)
        beta = rng.standard_normal(m) / np.sqrt(m)
        cols_t = torch.from_numpy(cols.astype(np.int64)).cuda()
        torch.cuda.synchronize()
        ms, tf = capi.op_info_bench(X, cols, repeats=a.repeats)
        rec = dict(base, what="information", case=name, n=n, p=p, m=m, gram_ms=ms, gram_tflops=tf, repeats=a.repeats,
                   share_of_fp64_matrix_peak=tf / PEAK_FP64_MATRIX_TFLOPS, workspace_doubles=capi.info_workspace(n, m)[0])

        def device():
            r = capi.information_device(X, cols, beta, 0.1, y, link="logistic", weight=w)
            return r["info"], r["score"]

        def torch_route():
            Xs = X[:, cols_t].to(torch.float64)
            eta = capi.predict_device(X, cols, beta, [0.1])
            pr = torch.sigmoid(eta)
            Z = torch.cat([torch.ones((n, 1), device="cuda", dtype=torch.float64), Xs], dim=1)
            info = Z.T @ (Z * (w * pr * (1 - pr))[:, None])
            score = Z.T @ (w * (y - pr))
            return info.cpu().numpy(), score.cpu().numpy()

        (ia, _), (ib, _) = device(), torch_route()  # warm-up of both, and the two routes must agree
        d = np.sqrt(np.diag(ib))
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
        del X
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
            print(json.dumps(ln))


if __name__ == "__main__":
    main()
