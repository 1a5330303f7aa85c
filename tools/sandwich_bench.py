"""The meat of the robust and cluster-robust covariances of one model on an X already on the GPU: sandwich_device against
the torch route it replaces.

  python tools/sandwich_bench.py [--repeats 20] [--calls 7] [--out profiles/sandwich_bench.jsonl]

Writes one JSON line per case.  Cases: the configs[1] shape (n = 50 000, p = 10 000) with a support of m = 200 columns as
fp64 column-major, fp64 row-major and fp32 row-major X (the layouts of tools/diag_bench.py), each for HC0 without
clusters, HC3 (a ready factor R, made outside the timed region), clusters of about 8 rows with sorted labels, and the same
clusters with shuffled labels.  Logistic link, weights.  Both routes end with info, score and the meat on the host:
  device     capi.sandwich_device(X, cols, beta, coef0, y_dev, link="logistic", weight=w_dev, kind=..., factor=R,
             cluster=labels)
  torch      what a user has without it: gather X[:, cols] into an n x m tensor, capi.predict_device for eta, the n x M
             score matrix u z, index_add_ over the labels (clustered) and two rocBLAS Grams (info and the meat); for HC3
             also Z @ R^T and the row sums of its squares
Per case:
  sums_ms              bessx_op_sandwich_bench (device events, one warm-up: the cluster-sum kernel alone and, for clusters
                       longer than a run, the addition of their partials); null without clusters
  sums_gbps            the bytes the algorithm needs (the support and u once, S once; not the kernel's re-reads of u,
                       the row order and the run table) / sums_ms;  share_of_copy_rate = sums_gbps / the device copy rate
                       measured in the same run (capi.op_stream_copy_gbps).  The repeated launches run over a working set
                       (about 90 MB for fp64) that fits the 256 MB last-level cache, the copy rate is an HBM figure: the
                       share is an upper estimate of what a cold call reaches
  device_ms, torch_ms  wall time to the host results, the two routes ALTERNATING, --calls each after one warm-up each:
                       median, and min / max as the spread
  torch_over_device    ratio of the medians
  max_rel_diff_of_the_routes   largest |difference| of a meat entry over the largest entry
  workspace_doubles    device scratch of the device route (capi.sandwich_workspace); torch_doubles: the n x m gather and
                       the n x M score matrix the torch route allocates
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
    ap.add_argument("--out", default=os.path.join("profiles", "sandwich_bench.jsonl"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("sandwich_bench: no GPU (nothing is measured on a CPU)")
    n, p, m = 50000, 10000, 200
    M = m + 1
    layouts = [("configs[1] fp64 column-major", torch.float64, True), ("configs[1] fp64 row-major", torch.float64, False),
               ("configs[1] fp32 row-major", torch.float32, False)]
    rng = np.random.default_rng(3)
    sizes = []
    while sum(sizes) < n:
        sizes.append(min(int(rng.integers(1, 16)), n - sum(sizes)))  # mean 8
    sorted_labels = np.repeat(np.arange(len(sizes), dtype=np.int64), sizes)
    shuffled_labels = rng.permutation(sorted_labels)
    cases = [("HC0", "HC0", None), ("HC3", "HC3", None), ("clusters of ~8, sorted labels", "HC1", sorted_labels),
             ("clusters of ~8, shuffled labels", "HC1", shuffled_labels)]
    copy_gbps = capi.op_stream_copy_gbps()
    base = {"device": capi.device_info(), "label": a.label, "copy_gbps": copy_gbps}
    lines = []
    for name, dt, colmajor in layouts:
        g = torch.Generator(device="cuda").manual_seed(1)
        X = torch.randn((n, p), generator=g, device="cuda", dtype=dt)
        if colmajor:
            X = X.T.contiguous().T
        y = (torch.rand((n,), generator=g, device="cuda", dtype=torch.float64) < 0.5).to(torch.float64)
        w = torch.rand((n,), generator=g, device="cuda", dtype=torch.float64) + 0.5
        cols = np.sort(rng.choice(p, m, replace=False)).astype(np.int32)
        beta = rng.standard_normal(m) / np.sqrt(m)
        cols_t = torch.from_numpy(cols.astype(np.int64)).cuda()
        info = capi.information_device(X, cols, beta, 0.1, y, link="logistic", weight=w)
        R, pd = capi.info_factor(info["info"])
        assert pd
        R_t = torch.from_numpy(R).cuda()
        torch.cuda.synchronize()
        for case, kind, labels in cases:
            G = None if labels is None else int(np.unique(labels).size)
            longest = 0 if labels is None else int(np.bincount(labels).max())
            ws = capi.sandwich_workspace(n, m, link="logistic", weighted=True, kind=kind, n_clusters=G or 0,
                                         max_cluster_rows=longest, dtype=np.float32 if dt == torch.float32 else np.float64,
                                         row_stride=X.stride(0), col_stride=X.stride(1))
            rec = dict(base, what="sandwich", layout=name, case=case, kind=kind, n=n, p=p, m=m, n_clusters=G,
                       repeats=a.repeats, workspace_doubles=ws["doubles"], torch_doubles=n * m + n * M,
                       sum_depth=ws["sum_depth"], sums_ms=None, sums_gbps=None, share_of_copy_rate=None)
            if labels is not None:
                ms, nbytes = capi.op_sandwich_bench(X, cols, labels, repeats=a.repeats)
                gbps = nbytes / (ms * 1e-3) / 1e9
                rec.update(sums_ms=ms, sums_gbps=gbps, share_of_copy_rate=gbps / copy_gbps)
                lab_t = torch.from_numpy(np.unique(labels, return_inverse=True)[1]).cuda()

            def device():
                return capi.sandwich_device(X, cols, beta, 0.1, y, link="logistic", weight=w, kind=kind,
                                            factor=R if kind == "HC3" else None, cluster=labels)

            def torch_route():
                Xs = X[:, cols_t].to(torch.float64)
                eta = capi.predict_device(X, cols, beta, [0.1])
                pr = torch.sigmoid(eta)
                Z = torch.cat([torch.ones((n, 1), device="cuda", dtype=torch.float64), Xs], dim=1)
                v = w * pr * (1 - pr)
                u = w * (y - pr)
                info_t = Z.T @ (v[:, None] * Z)
                if kind == "HC3":
                    T = Z @ R_t.T
                    u = u / (1 - v * (T * T).sum(dim=1))
                Y = u[:, None] * Z
                if labels is not None:
                    Y = torch.zeros((G, M), device="cuda", dtype=torch.float64).index_add_(0, lab_t, Y)
                return {"info": info_t.cpu().numpy(), "score": (Z.T @ (w * (y - pr))).cpu().numpy(),
                        "meat": (Y.T @ Y).cpu().numpy()}

            da, db = device(), torch_route()  # warm-up of both, and the two routes must agree
            torch.cuda.synchronize()
            rec.update(max_rel_diff_of_the_routes=float(np.abs(da["meat"] - db["meat"]).max() / np.abs(db["meat"]).max()))
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
