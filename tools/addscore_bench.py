"""Score tests of every excluded column against one model on an X already on the GPU: addscore_device against the
torch route it replaces.

  python tools/addscore_bench.py [--repeats 5] [--calls 7] [--out profiles/addscore_bench.jsonl]

Writes one JSON line per case.  Cases: the configs[1] shape (n = 50 000, p = 10 000) with a support of m = 200 columns,
all p columns as candidates, as fp64 column-major, fp64 row-major and fp32 row-major X.  Logistic link, weights, a ready
factor R (capi.info_factor of information_device's matrix, made outside the timed region).  Both routes end with the four
vectors u, d, s, a on the host:
  device     capi.addscore_device(X, cols, beta, coef0, y_dev, link="logistic", weight=w_dev, factor=R)
  torch      what a user has without it:
                 Xs = X[:, cols]                                  gather of the support (n x m)
                 eta = capi.predict_device(X, cols, beta, [coef0]);  p = sigmoid(eta);  v = w p (1 - p);  g = w (y - p)
                 Z = [1, Xs];  Pn = [v[:, None] * Z, g]            n x (M + 1)
                 D = X.T @ Pn                                     p x (M + 1), rocBLAS: C = D[:, :M], u = D[:, M]
                 d = (X * X).T @ v                                an X-SIZED temporary
                 T = C @ R.T;  s = (T * T).sum(1);  a = C @ (R.T @ (R @ (Z.T @ g)))
             For the fp32 X the route first makes the fp64 copy X.double() it needs for an fp64 result (another X-sized
             temporary, 2 x the bytes of X); the copy is inside the timed region, as it is for a user.
Per case:
  stage_ms             bessx_op_addscore_bench (device events, one warm-up): pack, cross, finish, statistic, each over
                       every block of candidates
  cross_tflops         2 n q Mp / cross ms, Mp = 16 ceil((m + 2) / 16);  share_of_matrix_peak = cross_tflops / 78.6
  cross_gbps           the bytes the cross kernel must move (n q item for X once per run of 8 panel tiles, the panel once
                       per four candidate tile rows, the partials once) / cross ms;  share_of_copy_rate = cross_gbps / the
                       device copy rate measured in the same run (capi.op_stream_copy_gbps)
  device_ms, torch_ms  wall time to the four host vectors, the two routes ALTERNATING, --calls each after one warm-up
                       each: median, and min / max as the spread
  torch_over_device    ratio of the medians
  device_peak_bytes, torch_peak_bytes   torch.cuda.max_memory_allocated over one call of the torch route (beyond what was
                       allocated before it) and the library's own scratch (capi.addscore_workspace doubles * 8: the
                       library allocates outside torch's allocator)
  max_rel_diff_of_the_routes   largest |difference| of u, d, s relative to the largest entry
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
    ap.add_argument("--out", default=os.path.join("profiles", "addscore_bench.jsonl"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("addscore_bench: no GPU (nothing is measured on a CPU)")
    n, p, m = 50000, 10000, 200
    M = m + 1
    Mp = 16 * ((M + 1 + 15) // 16)
    cases = [("configs[1] fp64 column-major", torch.float64, True), ("configs[1] fp64 row-major", torch.float64, False),
             ("configs[1] fp32 row-major", torch.float32, False)]
    copy_gbps = capi.op_stream_copy_gbps()
    base = {"device": capi.device_info(), "label": a.label, "copy_gbps": copy_gbps}
    ws = capi.addscore_workspace(n, m, p)
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
        st = capi.op_addscore_bench(X, cols, repeats=a.repeats)
        item = 4 if dt == torch.float32 else 8
        runs, tile_rows = (Mp // 16 + 7) // 8, (p + 15) // 16
        cross_bytes = (float(n) * p * item * runs + float(n) * Mp * 8 * ((tile_rows + 3) // 4)
                       + float(ws["slabs"]) * tile_rows * (Mp // 16 * 256 + 16) * 8)
        tf = 2.0 * n * p * Mp / (st["cross"] * 1e-3) / 1e12
        gbps = cross_bytes / (st["cross"] * 1e-3) / 1e9
        rec = dict(base, what="addscore", case=name, n=n, p=p, m=m, q=p, Mp=Mp, stage_ms=st, cross_tflops=tf,
                   share_of_matrix_peak=tf / MATRIX_PEAK_TFLOPS, cross_bytes=cross_bytes, cross_gbps=gbps,
                   share_of_copy_rate=gbps / copy_gbps, repeats=a.repeats, workspace=ws)

        def device():
            got = capi.addscore_device(X, cols, beta, 0.1, y, link="logistic", weight=w, factor=R)
            return got["u"], got["d"], got["s"], got["a"]

        def torch_route():
            Xd = X if X.dtype == torch.float64 else X.double()
            Xs = Xd[:, cols_t]
            eta = capi.predict_device(X, cols, beta, [0.1]).reshape(-1)
            pr = torch.sigmoid(eta)
            v, gg = w * pr * (1 - pr), w * (y - pr)
            Z = torch.cat([torch.ones((n, 1), device="cuda", dtype=torch.float64), Xs], dim=1)
            Pn = torch.cat([v[:, None] * Z, gg[:, None]], dim=1)
            D = Xd.T @ Pn
            C, u = D[:, :M], D[:, M]
            d = (Xd * Xd).T @ v
            T = C @ R_t.T
            s = (T * T).sum(dim=1)
            aa = C @ (R_t.T @ (R_t @ (Z.T @ gg)))
            return u.cpu().numpy(), d.cpu().numpy(), s.cpu().numpy(), aa.cpu().numpy()

        da, db = device(), torch_route()  # warm-up of both, and the two routes must agree
        torch.cuda.synchronize()
        rec.update(max_rel_diff_of_the_routes=max(float(np.abs(x - z).max() / np.abs(z).max()) for x, z in zip(da[:3], db[:3])))
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        torch_route()
        torch.cuda.synchronize()
        rec.update(torch_peak_bytes=int(torch.cuda.max_memory_allocated() - before))
        torch.cuda.reset_peak_memory_stats()
        device()
        torch.cuda.synchronize()
        rec.update(device_peak_bytes=int(torch.cuda.max_memory_allocated() - before) + 8 * int(ws["doubles"]))
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
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
            print(json.dumps(ln))


if __name__ == "__main__":
    main()
