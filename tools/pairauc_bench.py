"""The cumulative/dynamic AUC with Uno's C of the candidates of a Cox path, and the ROC AUC of the candidates of a
logistic path, on an X already on the GPU: the tiled pair kernel against the route a user has without it.

  python tools/pairauc_bench.py [--family cox logistic] [--p 2000] [--T 100] [--repeats 3] [--calls 7]
                                [--step-timeout 900] [--out profiles/pairauc_bench.jsonl]

The parent process only starts one child per case (family x layout of X x R), each under its own time limit, and stops
at the first child that fails; a child makes the design on the device (cox: the validation rows of configs[4], n = 200 000,
m = 150 support columns, T = 100 times, R = 1 and 150; logistic: configs[2], n = 100 000, m = 100, R = 1 and 100; fewer
columns than either), gives candidate r the first m - R + r + 1 support columns (a path: nested supports, the last one
full), measures, and appends one JSON line to --out.  Layouts of X: fp64 column-major, fp64 row-major, fp32 row-major.
Cox: distinct times, about 60% events, the T requested times are quantiles of the row times, Kaplan-Meier weights.
Per case:
  stage_ms               bessx_op_pairauc_bench (device events, one warm-up launch per stage): the predictor pass that
                         stores eta in position order, the pair kernel k_pa_pairs in AUC mode, its two finish kernels,
                         the pair kernel in Uno mode
  pairs, gpairs_s        the pairs (k, l) the AUC-mode launch compares, all models together, and that over its time
  fused_s, torch_s       wall time (host clock around work that ends in a device synchronise) of ONE capi.cox_auc_device /
                         capi.auc_device call for the R models and of the route it replaces -- per model
                         capi.predict_device on the model's own support, torch.sort of eta, then cumulative sums of the
                         controls' weights in that order (for Cox an n x T matrix per model) -- ALTERNATING, --calls each
                         after one warm-up each: median, min and max as the spread.  Both routes form the Kaplan-Meier
                         weights on the host inside the timed call.  The fused Cox call ALSO counts Uno's C (a second
                         O(n^2) launch, stage_ms[3]); the torch route does not compute it.
  max_rel_diff           of the two routes' AUCs
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
LAYOUTS = ("fp64 column-major", "fp64 row-major", "fp32 row-major")
SHAPES = {"cox": (200000, 150, (1, 150)), "logistic": (100000, 100, (1, 100))}  # n, m, R


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


def child(a, family, layout, R):
    import torch
    from bess_amd import capi
    if not torch.cuda.is_available():
        raise SystemExit("pairauc_bench: no GPU (nothing is measured on a CPU)")
    n, m, _ = SHAPES[family]
    p, T = a.p, (a.T if family == "cox" else 1)
    g = torch.Generator(device="cuda").manual_seed(1)
    dtype = torch.float32 if layout.startswith("fp32") else torch.float64
    if layout.endswith("column-major"):
        X = torch.randn((p, n), generator=g, device="cuda", dtype=dtype).T
    else:
        X = torch.randn((n, p), generator=g, device="cuda", dtype=dtype)
    torch.cuda.synchronize()
    rng = np.random.default_rng(3)
    cols = np.sort(rng.choice(p, m, replace=False)).astype(np.int32)
    B = np.zeros((m, R))
    for r in range(R):
        k = m - R + r + 1
        B[:k, r] = rng.standard_normal(k) / np.sqrt(k)
    tm = rng.permutation(n).astype(np.float64) + 1.0
    status = (rng.uniform(size=n) < 0.6).astype(np.float64)
    times = np.quantile(tm, (np.arange(T) + 0.5) / T * 0.8)
    y = (rng.uniform(size=n) < 0.4).astype(np.float64)
    zero = np.zeros(1)
    rec = {"device": capi.device_info(), "what": "pairauc", "family": family, "n": n, "p": p, "m": m, "T": T, "R": R,
           "source": layout, "label": a.label, "repeats": a.repeats, "calls": a.calls,
           "workspace_doubles": capi.cox_auc_workspace(n, T, R)[0]}
    ms, pairs = capi.op_pairauc_bench(X, cols, R=R, T=T, repeats=a.repeats)
    rec["stage_ms"], rec["pairs"], rec["gpairs_s"] = list(ms), pairs, pairs / (ms[1] * 1e-3) / 1e9
    d = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()

    def sorted_sums(eta, case_of, cw_d, w_d):
        """(greater, equal) per column of case_of(order): cumulative sums of the controls' weights in the order of eta."""
        es, oe = torch.sort(eta)
        new = torch.ones(n, dtype=torch.bool, device="cuda")
        new[1:] = es[1:] != es[:-1]
        gid = torch.cumsum(new, 0) - 1
        starts = torch.nonzero(new)[:, 0]
        ends = torch.cat([starts[1:], torch.tensor([n], device="cuda")])
        case = case_of(oe)  # n x T
        v = torch.where(case, 0.0, w_d[oe][:, None])
        cv = torch.cat([torch.zeros((1, v.shape[1]), dtype=torch.float64, device="cuda"), torch.cumsum(v, 0)])
        below, level = cv[starts][gid], (cv[ends] - cv[starts])[gid]
        u = torch.where(case, cw_d[oe][:, None], 0.0)
        return (u * below).sum(dim=0), (u * level).sum(dim=0)

    if family == "cox":
        def fused():
            return capi.cox_auc_device(X, cols, B, times, tm, status)["auc"]

        def torch_route():
            row_a = capi.ipcw_weights(tm, status, np.zeros(0))[0]  # (both routes form the weights on the host, per call)
            tm_d, a_d, t_d, w_d = d(tm), d(row_a), d(times), torch.ones(n, dtype=torch.float64, device="cuda")
            left = tm_d[:, None] <= t_d[None, :]
            den = (torch.where(left, a_d[:, None], 0.0).sum(dim=0) * (~left).sum(dim=0))
            out = torch.empty((T, R), dtype=torch.float64, device="cuda")
            for r in range(R):
                k = m - R + r + 1
                eta = capi.predict_device(X, cols[:k], B[:k, r], zero)
                gr, eq = sorted_sums(eta, lambda oe: left[oe], a_d, w_d)
                out[:, r] = (gr + 0.5 * eq) / den
            return out.cpu().numpy()
    else:
        def fused():
            return capi.auc_device(X, cols, B, y)["auc"].reshape(1, -1)

        def torch_route():
            y_d, w_d = d(y), torch.ones(n, dtype=torch.float64, device="cuda")
            pos = y_d > 0.5
            den = pos.sum() * (~pos).sum()
            out = torch.empty((1, R), dtype=torch.float64, device="cuda")
            for r in range(R):
                k = m - R + r + 1
                eta = capi.predict_device(X, cols[:k], B[:k, r], zero)
                gr, eq = sorted_sums(eta, lambda oe: pos[oe][:, None], w_d, w_d)
                out[:, r] = (gr + 0.5 * eq) / den
            return out.cpu().numpy()

    want, got = torch_route(), fused()
    rec["max_rel_diff"] = float(np.max(np.abs(want - got) / np.maximum(np.abs(want), 1e-300)))
    rec.update(_alternate({"fused": fused, "torch": torch_route}, a.calls, torch.cuda.synchronize))
    rec["torch_over_fused"] = rec["torch_s"] / rec["fused_s"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--family", nargs="+", default=["cox", "logistic"], choices=sorted(SHAPES))
    ap.add_argument("--layout", nargs="+", default=list(LAYOUTS), choices=LAYOUTS)
    ap.add_argument("--p", type=int, default=2000)
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--step-timeout", type=int, default=900)
    ap.add_argument("--label", default="this build")
    ap.add_argument("--out", default=os.path.join("profiles", "pairauc_bench.jsonl"))
    ap.add_argument("--case", nargs=3, metavar=("FAMILY", "LAYOUT", "R"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.case:
        child(a, a.case[0], a.case[1], int(a.case[2]))
        return
    passed = [x for x in sys.argv[1:]]
    for family in a.family:
        for layout in a.layout:
            for R in SHAPES[family][2]:
                cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__)] + passed + [
                    "--case", family, layout, str(R)]
                rc = subprocess.run(cmd).returncode
                if rc != 0:  # (a step that failed, faulted or ran out of time: nothing more is started on the GPU)
                    raise SystemExit("pairauc_bench: %s, %s, R = %d ended with status %d" % (family, layout, R, rc))


if __name__ == "__main__":
    main()
