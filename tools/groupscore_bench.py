"""Score tests of every excluded GROUP of columns against one model on an X already on the GPU: groupscore_device
against the torch route it replaces and against addscore_device (the column-by-column tests) on the same columns.

  python tools/groupscore_bench.py [--repeats 5] [--calls 7] [--out profiles/groupscore_bench.jsonl]

Writes one JSON line per case.  Cases: the configs[1] shape (n = 50 000, p = 10 000) with a support of m = 200 columns,
all p columns tested in groups of 5 and of 16 columns, as fp64 column-major, fp64 row-major and fp32 row-major X.  Logistic
link, weights, a ready factor R (capi.info_factor of information_device's matrix, made outside the timed region).  The
group routes end with u, a and the packed blocks D and S on the host, addscore_device with its four vectors:
  device     capi.groupscore_device(X, cols, beta, coef0, y_dev, starts, link="logistic", weight=w_dev, factor=R)
  torch      what a user has without it:
                 Xs = X[:, cols]                                  gather of the support (n x m)
                 eta = capi.predict_device(X, cols, beta, [coef0]);  p = sigmoid(eta);  v = w p (1 - p);  g = w (y - p)
                 Z = [1, Xs];  Pn = [v[:, None] * Z, g]            n x (M + 1)
                 Cu = X.T @ Pn                                    p x (M + 1), rocBLAS: C = Cu[:, :M], u = Cu[:, M]
                 B = X.view(n, G, d).permute(1, 0, 2);  D = bmm((v B)^T, B)     G x d x d, an X-SIZED temporary
                 T = (C @ R.T).view(G, d, M);  S = bmm(T, T^T);  a = C @ (R.T @ (R @ (Z.T @ g)))
             For the fp32 X the route first makes the fp64 copy X.double() it needs for an fp64 result; the copy is inside
             the timed region, as it is for a user.
  addscore   capi.addscore_device(X, cols, beta, coef0, y_dev, link="logistic", weight=w_dev, factor=R)
Per case:
  stage_ms             bessx_op_groupscore_bench (device events, one warm-up): pack, cross, finish, gram, gram_sum, s_band,
                       extract, each over every block of candidates
  gram_tflops          2 n q 16 (w + 1) / gram ms;  cross_tflops = 2 n q Mp / cross ms;  shares of the fp64 matrix peak
  device_ms, torch_ms, addscore_ms   wall time to the host arrays, the three routes ALTERNATING, --calls each after one
                       warm-up each: median, and min / max as the spread
  torch_over_device, device_over_addscore   ratios of the medians
  device_peak_bytes, torch_peak_bytes   torch.cuda.max_memory_allocated over one call of the torch route (beyond what was
                       allocated before it) and the library's own scratch (capi.groupscore_workspace doubles * 8)
  max_rel_diff_of_the_routes   largest |difference| of u, D, S relative to the largest entry
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--label", default="this build")
    ap.add_argument("--out", default=os.path.join("profiles", "groupscore_bench.jsonl"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("groupscore_bench: no GPU (nothing is measured on a CPU)")
    n, p, m = 50000, 10000, 200
    M = m + 1
    Mp = 16 * ((M + 1 + 15) // 16)
    layouts = [("fp64 column-major", torch.float64, True), ("fp64 row-major", torch.float64, False),
               ("fp32 row-major", torch.float32, False)]
    base = {"device": capi.device_info(), "label": a.label, "copy_gbps": capi.op_stream_copy_gbps()}
    lines = []
    for name, dt, colmajor in layouts:
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
        for d in (5, 16):
            G = p // d
            starts = np.arange(0, p, d, dtype=np.int32)
            ws = capi.groupscore_workspace(n, p, m, starts)
            st = capi.op_groupscore_bench(X, cols, starts, repeats=a.repeats)
            gtf = 2.0 * n * p * 16 * (ws["band"] + 1) / (st["gram"] * 1e-3) / 1e12
            ctf = 2.0 * n * p * Mp / (st["cross"] * 1e-3) / 1e12
            rec = dict(base, what="groupscore", case="configs[1] %s, groups of %d" % (name, d), n=n, p=p, m=m, q=p,
                       group_width=d, groups=G, Mp=Mp, stage_ms=st, gram_tflops=gtf,
                       gram_share_of_matrix_peak=gtf / MATRIX_PEAK_TFLOPS, cross_tflops=ctf,
                       cross_share_of_matrix_peak=ctf / MATRIX_PEAK_TFLOPS, repeats=a.repeats, workspace=ws)

            def device():
                got = capi.groupscore_device(X, cols, beta, 0.1, y, starts, link="logistic", weight=w, factor=R)
                return got["u"], got["D"], got["S"], got["a"]

            def torch_route():
                Xd = X if X.dtype == torch.float64 else X.double()
                Xs = Xd[:, cols_t]
                eta = capi.predict_device(X, cols, beta, [0.1]).reshape(-1)
                pr = torch.sigmoid(eta)
                v, gg = w * pr * (1 - pr), w * (y - pr)
                Z = torch.cat([torch.ones((n, 1), device="cuda", dtype=torch.float64), Xs], dim=1)
                Pn = torch.cat([v[:, None] * Z, gg[:, None]], dim=1)
                Cu = Xd.T @ Pn
                C, u = Cu[:, :M], Cu[:, M]
                B = Xd.reshape(n, G, d).permute(1, 0, 2)
                D = torch.bmm((B * v[None, :, None]).transpose(1, 2), B)
                T = (C @ R_t.T).reshape(G, d, M)
                S = torch.bmm(T, T.transpose(1, 2))
                aa = C @ (R_t.T @ (R_t @ (Z.T @ gg)))
                return u.cpu().numpy(), D.reshape(-1).cpu().numpy(), S.reshape(-1).cpu().numpy(), aa.cpu().numpy()

            def addscore():
                got = capi.addscore_device(X, cols, beta, 0.1, y, link="logistic", weight=w, factor=R)
                return got["u"], got["d"], got["s"], got["a"]

            da, db = device(), torch_route()  # warm-up, and the two routes must agree
            addscore()
            torch.cuda.synchronize()
            rec.update(max_rel_diff_of_the_routes=max(float(np.abs(x - z).max() / np.abs(z).max())
                                                      for x, z in zip(da[:3], db[:3])))
            before = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            torch_route()
            torch.cuda.synchronize()
            rec.update(torch_peak_bytes=int(torch.cuda.max_memory_allocated() - before))
            torch.cuda.reset_peak_memory_stats()
            device()
            torch.cuda.synchronize()
            rec.update(device_peak_bytes=int(torch.cuda.max_memory_allocated() - before) + 8 * int(ws["doubles"]))
            times = {"device": [], "torch": [], "addscore": []}
            for _ in range(a.calls):
                for leg, fn in (("device", device), ("torch", torch_route), ("addscore", addscore)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    times[leg].append((time.perf_counter() - t0) * 1e3)
            med = {k: statistics.median(v) for k, v in times.items()}
            for k, v in times.items():
                rec.update({k + "_ms": med[k], k + "_min_ms": min(v), k + "_max_ms": max(v)})
            rec.update(calls=a.calls, torch_over_device=med["torch"] / med["device"],
                       device_over_addscore=med["device"] / med["addscore"])
            lines.append(rec)
            torch.cuda.empty_cache()
        del X
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
            print(json.dumps(ln))


if __name__ == "__main__":
    main()
