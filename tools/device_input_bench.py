"""X already on the GPU: the ingest kernel alone, and tensor-on-device -> session-ready, against the host route.

  python tools/device_input_bench.py [--n 50000 --p 10000] [--repeats 20] [--sessions 3] [--out profiles/device_input_bench.jsonl]

Writes one JSON line per measurement.  For fp64 row-major, fp64 column-major and fp32 row-major X of the configs[1] shape:
  ingest_kernel     ms and GB/s (bytes read + written) of bessx_op_ingest_bench (device events, one warm-up launch, the
                    device otherwise idle), beside bessx_op_stream_copy_gbps measured in the same process
  session_ready     wall time from "a torch tensor on the device" to "capi.Session constructed" (host clock around work
                    that ends in a device synchronise): the device route, and the host route a user without it has to take
                    (X.cpu().numpy(), then capi.Session); median of --sessions runs after one warm-up each, and the ratio
--host-only runs just the host route (its code does not depend on the device route: the same leg can be timed on an
older build of the library).
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
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--p", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--sessions", type=int, default=3)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--label", default="this build")
    ap.add_argument("--out", default=os.path.join("profiles", "device_input_bench.jsonl"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("device_input_bench: no GPU (nothing is measured on a CPU)")
    n, p = a.n, a.p
    g = torch.Generator(device="cuda").manual_seed(1)
    X64 = torch.randn((n, p), generator=g, device="cuda", dtype=torch.float64)
    y = np.random.default_rng(2).standard_normal(n)
    shapes = {"fp64 row-major": lambda: X64, "fp64 column-major": lambda: X64.T.contiguous().T,
              "fp32 row-major": lambda: X64.to(torch.float32)}
    lines = []
    base = {"device": capi.device_info(), "n": n, "p": p, "label": a.label}
    copy = None
    if not a.host_only:
        copy = capi.op_stream_copy_gbps(1 << 31, 10)
        lines.append(dict(base, what="stream_copy", gbps=copy))
    for name, make in shapes.items():
        X = make()
        torch.cuda.synchronize()
        rec = dict(base, shape=name)
        if not a.host_only:
            ms, gbps = capi.op_ingest_bench(X, repeats=a.repeats)
            lines.append(dict(rec, what="ingest_kernel", ms=ms, gbps=gbps, fraction_of_stream_copy=gbps / copy,
                              repeats=a.repeats))

        def device_route():
            s = capi.Session(X, y)
            s.close()

        def host_route():
            s = capi.Session(X.cpu().numpy(), y)
            s.close()

        times = {}
        for leg, fn in (("host", host_route),) if a.host_only else (("device", device_route), ("host", host_route)):
            fn()  # warm-up
            ts = []
            for _ in range(a.sessions):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            times[leg] = ts
        out = dict(rec, what="session_ready", sessions=a.sessions,
                   host_route_s=statistics.median(times["host"]), host_route_all_s=times["host"])
        if not a.host_only:
            out.update(device_route_s=statistics.median(times["device"]), device_route_all_s=times["device"],
                       host_over_device=statistics.median(times["host"]) / statistics.median(times["device"]))
        lines.append(out)
        del X
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
            print(json.dumps(ln))


if __name__ == "__main__":
    main()
