"""Standard errors and confidence bands of the curves of a Cox model on an X already on the GPU, against the route a user
has without them.

  python tools/cox_band_bench.py [--n 200000 --p 2000] [--m 150] [--T 1 100] [--repeats 5] [--calls 7]
                                 [--step-timeout 300] [--out profiles/cox_band_bench.jsonl]

The parent process only starts one child per case (layout of X x T), each under its own time limit, and stops at the
first child that fails; a child makes the design on the device (the rows of configs[4], n = 200 000, fewer columns), draws
m = 150 support columns, fits nothing -- the model, the times and the status are drawn -- runs
capi.cox_information_device + capi.info_factor + capi.cox_baseline_variance_device once for the inputs of the band call,
measures, and appends one JSON line to --out.  Layouts of X: fp64 row-major, fp64 column-major, fp32 row-major.
Per case:
  stage_ms               bessx_op_cox_band_bench (device events, one warm-up launch per stage): the predictor pass that
                         stores exp(clip(eta)), k_cbd_band writing the estimate / lower / upper slabs
  band_tflops            2 n Mpad^2 / the time of k_cbd_band, Mpad = 16 ceil(m / 16): the flops of ONE formation of t = Z R^T
                         taken as dense (the kernel issues the lower half only, and once per chunk of times)
  copy_gbps              bessx_op_stream_copy_gbps (read + write bytes / time) in the same process
  band_slabs_gbps        3 n T 8 bytes written / the time of k_cbd_band; band_share_of_copy: that over copy_gbps
  fused_s, torch_s,      wall time (host clock around work that ends in a device synchronise) of
  torch_expanded_s       capi.cox_survival_band_device and of two routes a user has without it, both starting with the gather
                         X[:, cols], capi.predict_device, Z @ R.T and P = drift @ R.T and ending with the band formulas on
                         n x T tensors: "torch" forms |p_tau - H_tau t_i|^2 directly, one time at a time (T passes over an
                         n x m temporary); "torch_expanded" forms |p|^2 - 2 H p.t + H^2 |t|^2 with one more GEMM, the form
                         that cancels for columns that are not centred.  ALTERNATING, --calls each after one warm-up each:
                         median, min and max as the spread.  (torch.cdist with compute_mode
                         "donot_use_mm_for_euclid_dist" is not used: at n = 200 000, T = 100 it returned distances that are
                         off by up to 0.99 of V against a longdouble reference, where the fused route and the loop agree
                         with it to 1e-15.)
  max_abs_diff_...       largest difference of estimate / lower / upper between the fused route and each torch route
  hazard_var_s           one capi.cox_baseline_variance_device call (host sort included)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LAYOUTS = ("fp64 row-major", "fp64 column-major", "fp32 row-major")


def _alternate(legs, calls, sync):
    for fn in legs.values():  # one warm-up each
        fn()
    times = {k: [] for k in legs}
    for _ in range(calls):
        for k, fn in legs.items():
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            times[k].append(time.perf_counter() - t0)
    out = {}
    for k, v in times.items():
        out.update({k + "_s": statistics.median(v), k + "_min_s": min(v), k + "_max_s": max(v)})
    return out


def child(a, layout, T):
    import torch
    from bess_amd import capi
    if not torch.cuda.is_available():
        raise SystemExit("cox_band_bench: no GPU (nothing is measured on a CPU)")
    n, p, m = a.n, a.p, a.m
    g = torch.Generator(device="cuda").manual_seed(1)
    dtype = torch.float32 if layout.startswith("fp32") else torch.float64
    if layout.endswith("column-major"):
        X = torch.randn((p, n), generator=g, device="cuda", dtype=dtype).T
    else:
        X = torch.randn((n, p), generator=g, device="cuda", dtype=dtype)
    torch.cuda.synchronize()
    rng = np.random.default_rng(3)
    cols = np.sort(rng.choice(p, m, replace=False)).astype(np.int32)
    B = rng.standard_normal(m) / np.sqrt(m)
    tm = rng.permutation(n).astype(np.float64)
    status = (rng.uniform(size=n) < 0.5).astype(np.float64)
    zero = np.zeros(1)
    rec = {"device": capi.device_info(), "what": "cox_survival_band", "n": n, "p": p, "m": m, "T": T, "source": layout,
           "label": a.label, "repeats": a.repeats, "calls": a.calls}
    rec["stage_ms"] = list(capi.op_cox_band_bench(X, cols, T=T, repeats=a.repeats))
    mpad = 16 * ((m + 15) // 16)
    rec["band_tflops"] = 2.0 * n * mpad * mpad / (rec["stage_ms"][1] * 1e-3) / 1e12
    rec["copy_gbps"] = capi.op_stream_copy_gbps(1 << 28, 20)
    rec["band_slabs_gbps"] = 3.0 * n * T * 8.0 / (rec["stage_ms"][1] * 1e-3) / 1e9
    rec["band_share_of_copy"] = rec["band_slabs_gbps"] / rec["copy_gbps"]
    grid = np.quantile(tm, (np.arange(T) + 0.5) / T)
    info = capi.cox_information_device(X, cols, B, tm, status, ties="breslow")["info"]
    R, pd = capi.info_factor(info)
    if not pd:
        raise SystemExit("cox_band_bench: the information of the drawn model is not positive definite")
    t0 = time.perf_counter()
    hv = capi.cox_baseline_variance_device(X, cols, B, tm, status, grid)
    rec["hazard_var_s"] = time.perf_counter() - t0
    zc = capi.normal_quantile(0.95)
    H_d, V0_d = torch.from_numpy(hv["cumhaz"]).cuda(), torch.from_numpy(hv["var0"]).cuda()
    D_d, R_d = torch.from_numpy(hv["drift"]).cuda(), torch.from_numpy(R).cuda()
    cols_d = torch.from_numpy(cols.astype(np.int64)).cuda()

    def fused():
        return capi.cox_survival_band_device(X, cols, B, hv["cumhaz"], hv["var0"], hv["drift"], R)

    def bands(e, V):
        L = e[:, None] * H_d[None, :]
        r = zc * torch.sqrt(V) / H_d[None, :]
        return torch.stack([torch.exp(-L), torch.exp(-L * torch.exp(r)), torch.exp(-L * torch.exp(-r))])

    def operands():
        e = torch.exp(torch.clamp(capi.predict_device(X, cols, B, zero), -30.0, 30.0)).reshape(-1)
        Z = X[:, cols_d].double()                       # the n x m gathered copy
        return e, Z @ R_d.T, D_d @ R_d.T                # e (n,), t (n, m), P (T, m)

    def torch_direct():  # the direct form, one time at a time: T passes over an n x m temporary
        e, t, Pm = operands()
        V = torch.empty((n, T), dtype=torch.float64, device="cuda")
        for j in range(T):
            d = Pm[j][None, :] - H_d[j] * t
            V[:, j] = V0_d[j] + (d * d).sum(dim=1)
        return bands(e, V)

    def torch_expanded():  # the expansion |p|^2 - 2 H p.t + H^2 |t|^2: two GEMMs, cancels for columns that are not centred
        e, t, Pm = operands()
        S = (Pm * Pm).sum(dim=1)[None, :] - 2.0 * H_d[None, :] * (t @ Pm.T) + (H_d * H_d)[None, :] * (t * t).sum(dim=1)[:, None]
        return bands(e, V0_d[None, :] + torch.clamp(S, min=0.0))

    got = fused()
    for name, route in (("direct", torch_direct), ("expanded", torch_expanded)):
        want = route()
        rec["max_abs_diff_fused_vs_torch_" + name] = float(max((want[s] - got[k]).abs().max() for s, k in enumerate(got)))
        del want
    del got
    rec.update(_alternate({"fused": fused, "torch": torch_direct, "torch_expanded": torch_expanded}, a.calls,
                          torch.cuda.synchronize))
    rec["torch_over_fused"] = rec["torch_s"] / rec["fused_s"]
    rec["torch_expanded_over_fused"] = rec["torch_expanded_s"] / rec["fused_s"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--p", type=int, default=2000)
    ap.add_argument("--m", type=int, default=150)
    ap.add_argument("--T", type=int, nargs="+", default=[1, 100])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--label", default="this build")
    ap.add_argument("--out", default=os.path.join("profiles", "cox_band_bench.jsonl"))
    ap.add_argument("--case", nargs=2, metavar=("LAYOUT", "T"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.case:
        child(a, a.case[0], int(a.case[1]))
        return
    passed = [x for x in sys.argv[1:]]
    for layout in LAYOUTS:
        for T in a.T:
            cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__)] + passed + [
                "--case", layout, str(T)]
            rc = subprocess.run(cmd).returncode
            if rc != 0:  # (a step that failed, faulted or ran out of time: nothing more is started on the GPU)
                raise SystemExit("cox_band_bench: %s, T = %d ended with status %d" % (layout, T, rc))


if __name__ == "__main__":
    main()
