"""Prediction on an X already on the GPU: the kernel alone, est.predict(X_dev), and the host route.

  python tools/predict_bench.py [--n 50000 --p 10000] [--repeats 20] [--calls 5] [--out profiles/predict_bench.jsonl]

Writes one JSON line per case.  Sources: fp64 row-major, fp64 column-major and fp32 row-major X of the configs[1] shape;
supports m in {10, 100, 200} (columns drawn at random), R in {1, 64} responses (an LM estimator with beta (p,) or (p, R)).
Per case:
  kernel_ms          bessx_op_predict_bench (device events, one warm-up launch, the device otherwise idle)
  predict_device_s   wall time of est.predict(X_dev): host clock around work that ends in a device synchronise, median of
                     --calls after one warm-up
  predict_host_s     wall time of the route a user without the device entry has to take, est.predict(X_dev.cpu().numpy())
  bytes_used         n * m * item + n * R * 8: what the result needs
  column-major       gbps_used = bytes_used / kernel time, beside bessx_op_stream_copy_gbps of the same process
  row-major          the gather moves whole memory segments for 4- or 8-byte elements: segments_64B counts the distinct
                     64-byte segments of X the support touches in every row (computed from cols, the row stride and the
                     base alignment), bytes_touched = 64 * segments + n * R * 8; gbps_used and gbps_touched are both given,
                     and only gbps_touched is comparable with a memory rate
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bess_amd import capi, linear  # noqa: E402


def segments_per_row(cols, item, seg=64):
    """Distinct seg-byte segments that the support's elements touch in one row whose first element is seg-aligned."""
    return int(np.unique((np.asarray(cols, dtype=np.int64) * item) // seg).size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--p", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--label", default="this build")
    ap.add_argument("--out", default=os.path.join("profiles", "predict_bench.jsonl"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("predict_bench: no GPU (nothing is measured on a CPU)")
    n, p = a.n, a.p
    g = torch.Generator(device="cuda").manual_seed(1)
    X64 = torch.randn((n, p), generator=g, device="cuda", dtype=torch.float64)
    shapes = {"fp64 row-major": lambda: X64, "fp64 column-major": lambda: X64.T.contiguous().T,
              "fp32 row-major": lambda: X64.to(torch.float32)}
    base = {"device": capi.device_info(), "n": n, "p": p, "label": a.label}
    copy = capi.op_stream_copy_gbps(1 << 31, 10)
    lines = [dict(base, what="stream_copy", gbps=copy)]
    rng = np.random.default_rng(3)
    for name, make in shapes.items():
        X = make()
        torch.cuda.synchronize()
        item = X.element_size()
        for m in (10, 100, 200):
            cols = np.sort(rng.choice(p, m, replace=False)).astype(np.int32)
            for R in (1, 64):
                est = linear.PdasLm()
                est.p = p
                est.beta = np.zeros((p, R)) if R > 1 else np.zeros(p)
                est.beta[cols] = rng.standard_normal((m, R)) if R > 1 else rng.standard_normal(m)
                est.coef0 = rng.standard_normal(R) if R > 1 else 0.5
                ms, gbps = capi.op_predict_bench(X, cols, R=R, repeats=a.repeats)
                used = n * m * item + n * R * 8
                rec = dict(base, what="predict", source=name, m=m, R=R, kernel_ms=ms, repeats=a.repeats,
                           bytes_used=used, gbps_used=gbps)
                if name.endswith("column-major"):
                    rec.update(stream_copy_gbps=copy, gbps_used_over_stream_copy=gbps / copy)
                else:
                    aligned = X.data_ptr() % 64 == 0 and (X.stride(0) * item) % 64 == 0
                    seg = segments_per_row(cols, item)
                    touched = 64 * seg * n + n * R * 8
                    rec.update(segments_64B_per_row=seg, rows_start_on_a_segment=bool(aligned), bytes_touched=touched,
                               gbps_touched=touched / (ms * 1e-3) / 1e9, stream_copy_gbps=copy)
                times = {}
                for leg, fn in (("device", lambda: est.predict(X)), ("host", lambda: est.predict(X.cpu().numpy()))):
                    fn()  # warm-up
                    ts = []
                    for _ in range(a.calls if leg == "device" else min(a.calls, 2)):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        fn()
                        torch.cuda.synchronize()
                        ts.append(time.perf_counter() - t0)
                    times[leg] = ts
                rec.update(predict_device_s=statistics.median(times["device"]), predict_device_all_s=times["device"],
                           predict_host_s=statistics.median(times["host"]), predict_host_all_s=times["host"],
                           host_over_device=statistics.median(times["host"]) / statistics.median(times["device"]))
                lines.append(rec)
        del X
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
            print(json.dumps(ln))


if __name__ == "__main__":
    main()
