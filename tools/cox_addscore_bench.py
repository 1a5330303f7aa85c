"""Score tests of every excluded column against one Cox model on an X already on the GPU: cox_addscore_device against
the torch route it replaces.

  python tools/cox_addscore_bench.py [--n 200000 --p 20000 --m 150] [--repeats 3] [--calls 7]
                                     [--out profiles/cox_addscore_bench.jsonl]

Writes one JSON line per case.  Cases: the configs[4] shape (n = 200 000, p = q = 20 000) with a support of m = 150
columns, ties = "breslow" (tie groups of four), as fp64 column-major, fp64 row-major and fp32 row-major X, each with the
rows in a scattered order and once more with the rows already in time order.  A ready factor R (capi.info_factor of
cox_information_device's matrix, made outside the timed region).  Both routes end with the five vectors u, d, t, s, a on
the host:
  device     capi.cox_addscore_device(X, cols, beta, time, status, ties="breslow", factor=R)
  torch      what a user has without it, over candidate blocks of 2048 columns because the n x p suffix-scan
             temporaries do not fit next to X (the blocks are part of the route, and said so in every line):
                 order = argsort(time);  Xs = X[order][:, cols];  eta = capi.predict_device(X, cols, beta, [0])[order]
                 e, S0, dh, H, v, g, the risk-set means of the support, A, cc by flip / cumsum on n and n x m arrays
                 P = [v Xs - e A, g]                                   n x (m + 1)
                 per block:  XJ = X[order, j0:j1] (fp64 copy);  D = XJ.T @ P (rocBLAS);  d = (XJ * XJ).T @ v
                             S1 = flip(cumsum(flip(e XJ)));  t = (cc S1^2).sum(0)
                 s = |C R^T|^2, a = C r
Per case:
  stage_ms             bessx_op_cox_addscore_bench (device events, one warm-up): pack, cross, quad, quad_finish, finish,
                       statistic, each over every block of candidates
  cross_tflops         2 n q Mp / cross ms, Mp = 16 ceil((m + 2) / 16);  share_of_matrix_peak = cross_tflops / 78.6
  quad_gbps            the bytes k_cas_quad needs (the candidate columns once: n q item) / quad ms;  share_of_copy_rate =
                       quad_gbps / the device copy rate measured in the same run (capi.op_stream_copy_gbps)
  device_ms, torch_ms  wall time to the five host vectors, the two routes ALTERNATING, --calls each after one warm-up
                       each: median, and min / max as the spread;  torch_over_device = ratio of the medians
  device_scratch_bytes, torch_peak_bytes   the library's own scratch (capi.cox_addscore_workspace doubles * 8) and
                       torch.cuda.max_memory_allocated over one call of the torch route beyond what was allocated before
  max_rel_diff_of_the_routes   largest |difference| of u, d, t, s relative to the largest entry
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

MATRIX_PEAK_TFLOPS = 78.6  # fp64 matrix peak of the MI355X (profiles/README.md)
TORCH_BLOCK = 2048


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--p", type=int, default=20000)
    ap.add_argument("--m", type=int, default=150)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--label", default="this build")
    ap.add_argument("--out", default=os.path.join("profiles", "cox_addscore_bench.jsonl"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("cox_addscore_bench: no GPU (nothing is measured on a CPU)")
    n, p, m = a.n, a.p, a.m
    Mp = 16 * ((m + 2 + 15) // 16)
    copy_gbps = capi.op_stream_copy_gbps()
    base = {"device": capi.device_info(), "label": a.label, "copy_gbps": copy_gbps, "torch_candidate_block": TORCH_BLOCK}
    rng = np.random.default_rng(3)
    cols = np.sort(rng.choice(p, m, replace=False)).astype(np.int32)
    beta = rng.standard_normal(m) / np.sqrt(m)
    status = (rng.uniform(size=n) < 0.5).astype(np.float64)
    J = int(status.sum())
    ws = capi.cox_addscore_workspace(n, m, J, p)
    scattered = (np.arange(n, dtype=np.int64) * 7919 % n if np.gcd(7919, n) == 1 else rng.permutation(n))
    cols_t = torch.from_numpy(cols.astype(np.int64)).cuda()
    for name, dt, colmajor in (("fp64 column-major", torch.float64, True), ("fp64 row-major", torch.float64, False),
                               ("fp32 row-major", torch.float32, False)):
        g = torch.Generator(device="cuda").manual_seed(1)
        X = torch.randn((p, n) if colmajor else (n, p), generator=g, device="cuda", dtype=dt)
        if colmajor:
            X = X.T
        for rows_sorted in (False, True):
            rank = np.arange(n, dtype=np.int64) if rows_sorted else scattered
            tm = (rank // 4).astype(np.float64)  # tie groups of four
            info = capi.cox_information_device(X, cols, beta, tm, status, ties="breslow")
            R, pd = capi.info_factor(info["info"])
            assert pd
            R_t = torch.from_numpy(R).cuda()
            tm_t, st_t = torch.from_numpy(tm).cuda(), torch.from_numpy(status).cuda()
            torch.cuda.synchronize()
            stg, qbytes = capi.op_cox_addscore_bench(X, cols, sorted_rows=rows_sorted, repeats=a.repeats)
            tf = 2.0 * n * p * Mp / (stg["cross"] * 1e-3) / 1e12
            gbps = qbytes / (stg["quad"] * 1e-3) / 1e9
            rec = dict(base, what="cox_addscore", case="configs[4] " + name, rows_sorted=rows_sorted, n=n, p=p, m=m, q=p,
                       Mp=Mp, ties="breslow", stage_ms=stg, cross_tflops=tf, share_of_matrix_peak=tf / MATRIX_PEAK_TFLOPS,
                       quad_bytes=qbytes, quad_gbps=gbps, share_of_copy_rate=gbps / copy_gbps, repeats=a.repeats,
                       workspace=ws, device_scratch_bytes=8 * int(ws["doubles"]))

            def device():
                got = capi.cox_addscore_device(X, cols, beta, tm, status, ties="breslow", factor=R)
                return got["u"], got["d"], got["t"], got["s"], got["a"]

            def sfx(z):
                return torch.flip(torch.cumsum(torch.flip(z, [0]), 0), [0])

            def torch_route():
                order = torch.argsort(tm_t, stable=True)
                t_s, d_s = tm_t[order], st_t[order]
                new = torch.ones(n, dtype=torch.bool, device="cuda")
                new[1:] = t_s[1:] != t_s[:-1]
                idx = torch.arange(n, device="cuda")
                first = torch.cummax(torch.where(new, idx, torch.zeros_like(idx)), 0)[0]
                starts = torch.nonzero(new).reshape(-1)
                ends = torch.cat([starts[1:] - 1, torch.full((1,), n - 1, dtype=starts.dtype, device="cuda")])
                last = ends[torch.cumsum(new.to(torch.int64), 0) - 1]
                Xs = X[:, cols_t].double()[order]
                eta = capi.predict_device(X, cols, beta, [0.0]).reshape(-1)[order]
                e = torch.exp(torch.clamp(eta, -30.0, 30.0))
                S0pos = sfx(e)
                S0 = S0pos[first]
                h = d_s / S0
                dh = torch.zeros(n, dtype=torch.float64, device="cuda").index_add_(0, first, h)
                H = torch.cumsum(h, 0)[last]
                v = e * H
                gg = d_s - v
                us = sfx(e[:, None] * Xs) / S0pos[:, None]
                A = torch.cumsum(dh[:, None] * us, 0)
                Pn = torch.cat([v[:, None] * Xs - e[:, None] * A, gg[:, None]], dim=1)
                cc = dh / S0pos
                u, d, t = (torch.empty(p, dtype=torch.float64, device="cuda") for _ in range(3))
                C = torch.empty((p, m), dtype=torch.float64, device="cuda")
                for j0 in range(0, p, TORCH_BLOCK):
                    XJ = X[:, j0:j0 + TORCH_BLOCK][order].double()
                    D = XJ.T @ Pn
                    C[j0:j0 + TORCH_BLOCK], u[j0:j0 + TORCH_BLOCK] = D[:, :m], D[:, m]
                    d[j0:j0 + TORCH_BLOCK] = (XJ * XJ).T @ v
                    S1 = sfx(e[:, None] * XJ)
                    t[j0:j0 + TORCH_BLOCK] = (cc[:, None] * S1 * S1).sum(dim=0)
                T = C @ R_t.T
                s = (T * T).sum(dim=1)
                aa = C @ (R_t.T @ (R_t @ (Xs.T @ gg)))
                return tuple(z.cpu().numpy() for z in (u, d, t, s, aa))

            da, db = device(), torch_route()  # warm-up of both, and the two routes must agree
            torch.cuda.synchronize()
            rec.update(max_rel_diff_of_the_routes=max(float(np.abs(x - z).max() / np.abs(z).max())
                                                      for x, z in zip(da[:4], db[:4])))
            before = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            torch_route()
            torch.cuda.synchronize()
            rec.update(torch_peak_bytes=int(torch.cuda.max_memory_allocated() - before))
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
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(rec) + "\n")
            print(json.dumps(rec), flush=True)
        del X
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
