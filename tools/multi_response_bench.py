"""Many responses against configs[1] (LM n=50000 p=10000, sequence 1..200): bessx_session_sequential_path_multi (the
responses as chains of ONE merged run on one Gram column cache) against the per-response loop of sequential_path.

Y's column 0 is the benchmark's y; the other columns alternate fresh signals on random supports and permutations of y.
For every R: ms of the batched call (second call on the session: the first creates the chain contexts), candidates per
second over all responses, union fills, responses the host finished through the ordinary path (counter 34: takeovers;
at R = 1 the one response, which always takes the ordinary path).  The loop runs on the SAME session: each response
installed in turn (set_responses with that one column, then sequential_path_multi, which runs one response through the
ordinary sequential_path; the upload of the column is not timed), every column of the largest R measured.
One JSON line per R.   python tools/multi_response_bench.py [--no-loop] [R ...]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bess_amd import capi, synth  # noqa: E402

args = sys.argv[1:]
loop = "--no-loop" not in args
Rs = [int(v) for v in args if v != "--no-loop"] or [1, 8, 64, 256]
n, p, kmax = 50000, 10000, 200
X, y, _, _ = synth.make_lm(n, p, 100)
seq = np.arange(1, kmax + 1)
rng = np.random.default_rng(2024)
Y = np.empty((n, max(Rs)))
Y[:, 0] = y
for r in range(1, Y.shape[1]):
    if r % 2 == 0:
        Y[:, r] = rng.permutation(y)
    else:
        sup = rng.choice(p, 100, replace=False)
        Y[:, r] = X[:, sup] @ rng.uniform(1.0, 100.0, sup.size) + rng.standard_normal(n)

with capi.Session(X, y, score_mode=2) as s:
    loop_ms = []
    if loop:
        s.set_responses(Y[:, :1])
        s.sequential_path_multi(seq, ic_type=3)  # (warm-up: the chunk chains' contexts)
        for r in range(Y.shape[1]):
            s.set_responses(Y[:, r:r + 1])
            t0 = time.perf_counter()
            s.sequential_path_multi(seq, ic_type=3)
            loop_ms.append((time.perf_counter() - t0) * 1e3)
    for R in Rs:
        s.set_responses(Y[:, :R])
        s.sequential_path_multi(seq, ic_type=3)  # (creates the chain contexts)
        c0 = s.counters()
        t0 = time.perf_counter()
        out = s.sequential_path_multi(seq, ic_type=3)
        ms = (time.perf_counter() - t0) * 1e3
        c1 = s.counters()
        ncand = sum(int(o["n_candidates"]) for o in out)
        line = {"R": R, "batched_ms": round(ms, 2), "batched_candidates_per_s": round(ncand / (ms / 1e3), 1),
                "union_fills": c1["multi_union_fills"] - c0["multi_union_fills"],
                "batched_responses": c1["multi_responses_batched"] - c0["multi_responses_batched"],
                "host_finished_responses": c1["multi_responses_host"] - c0["multi_responses_host"],
                "column0_best_T0": int(out[0]["best_T0"])}
        if loop:
            loop_total = float(np.sum(loop_ms[:R]))
            line.update({"loop_ms": round(loop_total, 2), "loop_candidates_per_s": round(ncand / (loop_total / 1e3), 1),
                         "speedup": round(loop_total / ms, 3)})
        print(json.dumps(line), flush=True)
