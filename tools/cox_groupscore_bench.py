"""Score tests of every excluded GROUP of columns against one Cox model on an X already on the GPU:
cox_groupscore_device against the torch route it replaces and against the column-by-column call.

  python tools/cox_groupscore_bench.py [--n 200000 --p 20000 --m 150] [--widths 5,16] [--repeats 3] [--calls 7]
                                       [--out profiles/cox_groupscore_bench.jsonl]

Writes one JSON line per case.  Cases: section 4l's shape (n = 200 000, p = q = 20 000, m = 150, ties = "breslow", tie
groups of four), all columns tested in groups of 5 and of 16, as fp64 column-major, fp64 row-major and fp32 row-major X,
each with the rows in a scattered order and once more with the rows already in time order.  A ready factor R
(capi.info_factor of cox_information_device's matrix, made outside the timed region).  All routes end on the host:
  device     capi.cox_groupscore_device(X, cols, beta, time, status, starts, ties="breslow", factor=R): u, a, D, T, S
  torch      what a user has without it, over candidate blocks of at most 2048 columns that hold whole groups because the
             n x q suffix-scan temporaries do not fit next to X (the blocks are part of the route):
                 order, e, S0, dh, H, v, g, A, cc and the panel Pn as in tools/cox_addscore_bench.py (gather,
                 capi.predict_device, flip / cumsum on n and n x m arrays)
                 per block:  XJ = X[order, j0:j1] (fp64 copy);  [C, u] = XJ.T @ Pn (rocBLAS)
                             D = bmm over XJ.view(n, G, d);  S1 = flip(cumsum(flip(e XJ)));  T = bmm over S1.view(n, G, d)
                 S = bmm over (C R^T).view(G, d, m),  a = C r
  columns    capi.cox_addscore_device on the same columns (u, d, t, s, a: one degree of freedom per column)
Per case:
  stage_ms             bessx_op_cox_groupscore_bench (device events, one warm-up): pack, cross, finish, gram, gram_sum,
                       s_band, extract, t_band, t_finish, each over every block of candidates
  t_tflops             the matrix instructions k_cgs_band executes (512 n per band tile) / t_band ms;
                       share_of_matrix_peak = t_tflops / 78.6
  t_gbps               the bytes the band of T needs (the tested columns once: n q item) / t_band ms;  share_of_copy_rate =
                       t_gbps / the device copy rate measured in the same run (capi.op_stream_copy_gbps)
  device_ms, torch_ms, columns_ms   wall time to the host arrays, the three routes ALTERNATING, --calls each after one
                       warm-up each: median, and min / max as the spread;  torch_over_device = ratio of the medians
  device_scratch_bytes, torch_peak_bytes   the library's own scratch (capi.cox_groupscore_workspace doubles * 8) and
                       torch.cuda.max_memory_allocated over one call of the torch route beyond what was allocated before
  max_rel_diff_of_the_routes   largest |difference| of u, D, T, S between device and torch relative to the largest entry
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
    ap.add_argument("--widths", default="5,16")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--label", default="this build")
    ap.add_argument("--out", default=os.path.join("profiles", "cox_groupscore_bench.jsonl"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("cox_groupscore_bench: no GPU (nothing is measured on a CPU)")
    n, p, m = a.n, a.p, a.m
    widths = [int(w) for w in a.widths.split(",")]
    assert all(p % d == 0 for d in widths), "every width must divide p"
    copy_gbps = capi.op_stream_copy_gbps()
    base = {"device": capi.device_info(), "label": a.label, "copy_gbps": copy_gbps}
    rng = np.random.default_rng(3)
    cols = np.sort(rng.choice(p, m, replace=False)).astype(np.int32)
    beta = rng.standard_normal(m) / np.sqrt(m)
    status = (rng.uniform(size=n) < 0.5).astype(np.float64)
    J = int(status.sum())
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
            for d in widths:
                starts = np.arange(0, p, d, dtype=np.int32)
                G = starts.size
                ws = capi.cox_groupscore_workspace(n, p, m, J, starts)
                tblock = TORCH_BLOCK // d * d
                torch.cuda.synchronize()
                stg, qbytes = capi.op_cox_groupscore_bench(X, cols, starts, sorted_rows=rows_sorted, repeats=a.repeats)
                bf = ws["block_first"]  # (the library's blocks hold whole groups)
                tiles = sum(((bf[b + 1] - bf[b]) * d + 15) // 16 for b in range(ws["blocks"])) * (ws["band"] + 1)
                tf = 512.0 * n * tiles / (stg["t_band"] * 1e-3) / 1e12
                gbps = qbytes / (stg["t_band"] * 1e-3) / 1e9
                rec = dict(base, what="cox_groupscore", case="section 4l " + name, rows_sorted=rows_sorted, n=n, p=p, m=m,
                           q=p, group_width=d, groups=G, ties="breslow", stage_ms=stg, t_tflops=tf,
                           share_of_matrix_peak=tf / MATRIX_PEAK_TFLOPS, t_bytes=qbytes, t_gbps=gbps,
                           share_of_copy_rate=gbps / copy_gbps, repeats=a.repeats, workspace=ws,
                           device_scratch_bytes=8 * int(ws["doubles"]), torch_candidate_block=tblock)

                def device():
                    got = capi.cox_groupscore_device(X, cols, beta, tm, status, starts, ties="breslow", factor=R)
                    return got["u"], got["D"], got["T"], got["S"], got["a"]

                def columns():
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
                    heads = torch.nonzero(new).reshape(-1)
                    ends = torch.cat([heads[1:] - 1, torch.full((1,), n - 1, dtype=heads.dtype, device="cuda")])
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
                    u = torch.empty(p, dtype=torch.float64, device="cuda")
                    C = torch.empty((p, m), dtype=torch.float64, device="cuda")
                    D, T = (torch.empty((G, d, d), dtype=torch.float64, device="cuda") for _ in range(2))
                    for j0 in range(0, p, tblock):
                        XJ = X[:, j0:j0 + tblock][order].double()
                        qb = XJ.shape[1]
                        Dm = XJ.T @ Pn
                        C[j0:j0 + qb], u[j0:j0 + qb] = Dm[:, :m], Dm[:, m]
                        Gv = XJ.view(n, qb // d, d).permute(1, 0, 2)  # (groups, n, d)
                        D[j0 // d:(j0 + qb) // d] = torch.bmm(Gv.transpose(1, 2), v[None, :, None] * Gv)
                        S1 = sfx(e[:, None] * XJ).view(n, qb // d, d).permute(1, 0, 2)
                        T[j0 // d:(j0 + qb) // d] = torch.bmm(S1.transpose(1, 2), cc[None, :, None] * S1)
                    TC = (C @ R_t.T).view(G, d, m)
                    S = torch.bmm(TC, TC.transpose(1, 2))
                    aa = C @ (R_t.T @ (R_t @ (Xs.T @ gg)))
                    return tuple(z.reshape(-1).cpu().numpy() for z in (u, D, T, S, aa))

                da, db = device(), torch_route()  # warm-up of both, and the two routes must agree
                columns()
                torch.cuda.synchronize()
                rec.update(max_rel_diff_of_the_routes=max(float(np.abs(x - z).max() / np.abs(z).max())
                                                          for x, z in zip(da[:4], db[:4])))
                before = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                torch_route()
                torch.cuda.synchronize()
                rec.update(torch_peak_bytes=int(torch.cuda.max_memory_allocated() - before))
                times = {"device": [], "torch": [], "columns": []}
                for _ in range(a.calls):
                    for leg, fn in (("device", device), ("torch", torch_route), ("columns", columns)):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        fn()
                        torch.cuda.synchronize()
                        times[leg].append((time.perf_counter() - t0) * 1e3)
                for leg, ts in times.items():
                    rec.update({leg + "_ms": statistics.median(ts), leg + "_min_ms": min(ts), leg + "_max_ms": max(ts)})
                rec.update(calls=a.calls, torch_over_device=rec["torch_ms"] / rec["device_ms"],
                           device_over_columns=rec["device_ms"] / rec["columns_ms"])
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(json.dumps(rec) + "\n")
                print(json.dumps(rec), flush=True)
        del X
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
