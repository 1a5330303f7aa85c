"""Leverage, residuals and Cook's distance of one model on an X already on the GPU: diagnostics_device against the torch
route it replaces.

  python tools/diag_bench.py [--repeats 20] [--calls 7] [--out profiles/diag_bench.jsonl]

Writes one JSON line per case.  Cases: the configs[1] shape (n = 50 000, p = 10 000) with a support of m = 200 columns as
fp64 column-major, fp64 row-major and fp32 row-major X, each for all seven kinds and for the leverage alone.  Logistic
link, weights, a ready factor R (capi.info_factor of information_device's matrix, made outside the timed region).  Both
routes end with the result tensors on the device:
  device     capi.diagnostics_device(X, cols, beta, coef0, y_dev, factor=R, link="logistic", weight=w_dev, kinds=...)
  torch      what a user has without it: gather X[:, cols] into an n x m tensor, capi.predict_device for eta, Z @ R^T
             (rocBLAS), the row sums of its squares, and the elementwise formulas
Per case:
  lev_ms               bessx_op_diag_bench (device events, one warm-up: k_diag_lev alone, all of its outputs)
  lev_gbps             the bytes it must move (n m item + 7 n 8 + the packed factor) / lev_ms;  share_of_copy_rate =
                       lev_gbps / the device copy rate measured in the same run (capi.op_stream_copy_gbps)
  lev_tflops           n Mpad^2 operations / lev_ms, Mpad = 16 ceil((m + 1) / 16)
  device_ms, torch_ms  wall time to the result tensors, the two routes ALTERNATING, --calls each after one warm-up each:
                       median, and min / max as the spread
  torch_over_device    ratio of the medians
  max_abs_diff_of_the_routes   largest |difference| of a leverage
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
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--label", default="this build")
    ap.add_argument("--out", default=os.path.join("profiles", "diag_bench.jsonl"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("diag_bench: no GPU (nothing is measured on a CPU)")
    n, p, m = 50000, 10000, 200
    cases = [("configs[1] fp64 column-major", torch.float64, True), ("configs[1] fp64 row-major", torch.float64, False),
             ("configs[1] fp32 row-major", torch.float32, False)]
    copy_gbps = capi.op_stream_copy_gbps()
    base = {"device": capi.device_info(), "label": a.label, "copy_gbps": copy_gbps}
    lines = []
    for name, dt, colmajor in cases:
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
        info = capi.information_device(X, cols, beta, 0.1, y, link="logistic", weight=w)
        R, pd = capi.info_factor(info["info"])
        assert pd
        R_t = torch.from_numpy(R).cuda()
        torch.cuda.synchronize()
        ms, tf, nbytes = capi.op_diag_bench(X, cols, repeats=a.repeats)
        gbps = nbytes / (ms * 1e-3) / 1e9
        for kinds in (capi.DIAG_KINDS, ("leverage",)):
            rec = dict(base, what="diagnostics", case=name, kinds="all" if len(kinds) > 1 else "leverage", n=n, p=p, m=m,
                       lev_ms=ms, lev_tflops=tf, lev_gbps=gbps, share_of_copy_rate=gbps / copy_gbps, repeats=a.repeats,
                       workspace_doubles=capi.diag_workspace(n, m, kinds))

            def device():
                return capi.diagnostics_device(X, cols, beta, 0.1, y, factor=R, link="logistic", weight=w, kinds=kinds)

            def torch_route():
                Xs = X[:, cols_t].to(torch.float64)
                eta = capi.predict_device(X, cols, beta, [0.1])
                pr = torch.sigmoid(eta)
                V = pr * (1 - pr)
                Z = torch.cat([torch.ones((n, 1), device="cuda", dtype=torch.float64), Xs], dim=1)
                T = Z @ R_t.T
                h = (w * V) * (T * T).sum(dim=1)
                out = {"leverage": h}
                if len(kinds) > 1:
                    r = y - pr
                    rp = torch.sqrt(w) * r / torch.sqrt(V)
                    f = torch.clamp(eta, min=0) + torch.log1p(torch.exp(-eta.abs())) - y * eta
                    rd = torch.sign(r) * torch.sqrt(w * torch.clamp(2 * (f + torch.xlogy(y, y) + torch.xlogy(1 - y, 1 - y)), min=0))
                    den = torch.sqrt(1 - h)
                    out.update(response=r, pearson=rp, deviance=rd, std_pearson=rp / den, std_deviance=rd / den,
                               cooks=rp * rp * h / ((m + 1) * (1 - h) ** 2))
                return out

            da, db = device(), torch_route()  # warm-up of both, and the two routes must agree
            torch.cuda.synchronize()
            rec.update(max_abs_diff_of_the_routes=float((da["leverage"] - db["leverage"]).abs().max()))
            times = {"device": [], "torch": []}
            for _ in range(a.calls):
                for leg, fn in (("device", device), ("torch", torch_route)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    times[leg].append((time.perf_counter() - t0) * 1e3)
            md, mt = statistics.median(times["device"]), statistics.median(times["torch"])
            rec.update(device_ms=md, device_min_ms=min(times["device"]), device_max_ms=max(times["device"]), torch_ms=mt,
                       torch_min_ms=min(times["torch"]), torch_max_ms=max(times["torch"]), calls=a.calls,
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
