"""Held-out loss of R models on an X already on the GPU: the fused evaluation against predict-then-reduce.

  python tools/eval_bench.py [--n 50000 --p 10000] [--m 200] [--repeats 20] [--calls 9] [--out profiles/eval_bench.jsonl]

Writes one JSON line per case.  Sources: fp64 row-major, fp64 column-major and fp32 row-major X of the configs[1] shape;
a support of m = 200 columns (drawn at random); R = 1 and R = 200 models (LM loss, one y shared by the models, weights).
Both routes end with R numbers on the host:
  fused      capi.evaluate_device(X, cols, B, coef0, y_dev, weight=w_dev): one pass over the support's columns
  baseline   what a user has without it: capi.predict_device into an n x R device tensor, then the loss and the sum as
             torch operations on the device, then .cpu()
Per case:
  kernel_ms            bessx_op_eval_bench (device events, one warm-up launch; the fused pass plus the addition of its
                       partials)
  bytes_used           n * m * item + n * 8 * 2: what the result needs;  gbps_used = bytes_used / kernel time
  column-major         gbps_used_over_stream_copy: the fraction of bessx_op_stream_copy_gbps of the same process
  row-major            the gather moves whole 64-byte segments: bytes_touched and gbps_touched as in predict_bench.py
  fused_s, baseline_s  wall time (host clock around work that ends with the numbers on the host), the two routes
                       ALTERNATING, --calls each after one warm-up each: median, and min / max as the spread
  baseline_over_fused  ratio of the medians;  fused_not_slower: the fused median is the smaller one, or the medians
                       differ by no more than the larger of the two spreads (max - min)
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


def segments_per_row(cols, item, seg=64):
    """Distinct seg-byte segments that the support's elements touch in one row whose first element is seg-aligned."""
    return int(np.unique((np.asarray(cols, dtype=np.int64) * item) // seg).size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--p", type=int, default=10000)
    ap.add_argument("--m", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--label", default="this build")
    ap.add_argument("--out", default=os.path.join("profiles", "eval_bench.jsonl"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench: no GPU (nothing is measured on a CPU)")
    n, p, m = a.n, a.p, a.m
    g = torch.Generator(device="cuda").manual_seed(1)
    X64 = torch.randn((n, p), generator=g, device="cuda", dtype=torch.float64)
    y = torch.randn((n,), generator=g, device="cuda", dtype=torch.float64)
    w = torch.rand((n,), generator=g, device="cuda", dtype=torch.float64) + 0.5
    shapes = {"fp64 row-major": lambda: X64, "fp64 column-major": lambda: X64.T.contiguous().T,
              "fp32 row-major": lambda: X64.to(torch.float32)}
    base = {"device": capi.device_info(), "n": n, "p": p, "label": a.label}
    copy = capi.op_stream_copy_gbps(1 << 31, 10)
    lines = [dict(base, what="stream_copy", gbps=copy)]
    rng = np.random.default_rng(3)
    cols = np.sort(rng.choice(p, m, replace=False)).astype(np.int32)
    for name, make in shapes.items():
        X = make()
        torch.cuda.synchronize()
        item = X.element_size()
        for R in (1, 200):
            B = rng.standard_normal((m, R)) / np.sqrt(m)
            c0 = rng.standard_normal(R)
            ms, gbps = capi.op_eval_bench(X, cols, R=R, repeats=a.repeats)
            used = n * m * item + n * 8 * 2
            rec = dict(base, what="evaluate", source=name, m=m, R=R, kernel_ms=ms, repeats=a.repeats, bytes_used=used,
                       gbps_used=gbps, stream_copy_gbps=copy)
            if name.endswith("column-major"):
                rec.update(gbps_used_over_stream_copy=gbps / copy)
            else:
                seg = segments_per_row(cols, item)
                touched = 64 * seg * n + n * 8 * 2
                rec.update(segments_64B_per_row=seg, bytes_touched=touched,
                           gbps_touched=touched / (ms * 1e-3) / 1e9,
                           gbps_touched_over_stream_copy=touched / (ms * 1e-3) / 1e9 / copy)

            def fused():
                return capi.evaluate_device(X, cols, B, c0, y, weight=w)["loss"]

            def baseline():
                eta = capi.predict_device(X, cols, B, c0)
                return (w[:, None] * (y[:, None] - eta) ** 2).sum(dim=0).cpu().numpy()

            lf, lb = fused(), baseline()  # warm-up of both, and the two routes must agree
            rec.update(max_rel_diff_of_the_routes=float(np.max(np.abs(lf - lb) / np.abs(lb))))
            times = {"fused": [], "baseline": []}
            for _ in range(a.calls):
                for leg, fn in (("fused", fused), ("baseline", baseline)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    times[leg].append(time.perf_counter() - t0)
            mf, mb = statistics.median(times["fused"]), statistics.median(times["baseline"])
            spread = max(max(v) - min(v) for v in times.values())
            rec.update(fused_s=mf, fused_min_s=min(times["fused"]), fused_max_s=max(times["fused"]),
                       baseline_s=mb, baseline_min_s=min(times["baseline"]), baseline_max_s=max(times["baseline"]),
                       calls=a.calls, baseline_over_fused=mb / mf, fused_not_slower=bool(mf <= mb or mf - mb <= spread))
            lines.append(rec)
        del X
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
            print(json.dumps(ln))


if __name__ == "__main__":
    main()
