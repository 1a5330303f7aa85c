"""The chunk chains' planning arithmetic (bess_amd/csrc/bessx_kplan.h: chunk bounds, coarse plan, the stitch round's
decision), compiled on its own -- the header includes the standard library only -- and compared with the formulas of
sequential_path_chunked restated here in Python.  No GPU."""
import bisect
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bess_amd", "csrc")

PROGRAM = r"""
#include "bessx_kplan.h"
#include <cstdio>
#include <iostream>
#include <string>
// stdin, one case per line:  B lm ns C wdiv seq[ns]  |  P C M  |  S C need[C] (m len met)[C]
// stdout, one line per case: B bounds[C + 1]  |  P coarse_at.. / start_of[C]  |  S changed[C] / any give_up_from / need[C]
int main() {
  std::string what;
  while (std::cin >> what) {
    if (what == "B") {
      int lm, ns, C;
      double wdiv;
      std::cin >> lm >> ns >> C >> wdiv;
      std::vector<int> seq((size_t)ns);
      for (int &v : seq) std::cin >> v;
      for (int b : bessx::chunk_bounds(lm != 0, seq.data(), ns, C, wdiv)) std::printf("%d ", b);
    } else if (what == "P") {
      int C, M;
      std::cin >> C >> M;
      const bessx::CoarsePlan pl = bessx::coarse_plan(C, M);
      for (int v : pl.coarse_at) std::printf("%d ", v);
      std::printf("/ ");
      for (int v : pl.start_of) std::printf("%d ", v);
    } else {
      int C;
      std::cin >> C;
      std::vector<char> need((size_t)C);
      std::vector<bessx::StitchRefit> refit((size_t)C);
      for (char &v : need) {
        int x;
        std::cin >> x;
        v = (char)x;
      }
      for (auto &t : refit) {
        int met;
        std::cin >> t.m >> t.len >> met;
        t.met = met != 0;
      }
      const bessx::StitchRound d = bessx::stitch_round(need, refit);
      for (char v : d.changed) std::printf("%d ", (int)v);
      std::printf("/ %d %d / ", d.any ? 1 : 0, d.give_up_from);
      for (char v : d.need) std::printf("%d ", (int)v);
    }
    std::printf("\n");
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("kplan")
    src, exe = str(d / "kplan_main.cpp"), str(d / "kplan_main")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-I", CSRC, src, "-o", exe])

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
        got = out.stdout.splitlines()
        assert len(got) == len(lines)
        return got

    return run


def ints(text):
    return [int(v) for v in text.split()]


def bounds_expected(lm, seq, C, wdiv):
    """sequential_path_chunked: LM ns * r / C; otherwise the split of the cumulative weights 1 + level / wdiv."""
    ns = len(seq)
    bounds = [0] * (C + 1)
    if lm:
        for r in range(1, C + 1):
            bounds[r] = ns * r // C
        return bounds
    tot, cum = 0.0, [0.0] * (ns + 1)
    for i in range(ns):
        tot += 1.0 + float(seq[i]) / wdiv
        cum[i + 1] = tot
    for r in range(1, C):
        b = bisect.bisect_left(cum, tot * r / C)  # std::lower_bound
        bounds[r] = min(max(b, bounds[r - 1] + 1), ns - (C - r))
    bounds[C] = ns
    return bounds


@pytest.mark.parametrize("mode", ["lm", "1e9", "160", "1"])
def test_chunk_bounds(planner, mode):
    lm, wdiv = mode == "lm", 1e9 if mode == "lm" else float(mode)
    cases = []
    for ns in (2, 3, 7, 64, 200):
        for C in (2, 3, 4, 8, 10):
            if C <= ns:
                cases += [(list(range(1, ns + 1)), C), (list(range(2, 2 * ns + 1, 2)), C)]
    got = planner(["B %d %d %d %r %s" % (lm, len(seq), C, wdiv, " ".join(map(str, seq))) for seq, C in cases])
    assert len(cases) == 32
    for (seq, C), line in zip(cases, got):
        b = ints(line)
        assert b == bounds_expected(lm, seq, C, wdiv), (mode, len(seq), C, seq[:2])
        assert b[0] == 0 and b[-1] == len(seq) and all(x < y for x, y in zip(b, b[1:])), (mode, len(seq), C, b)


def test_coarse_plan(planner):
    cases = [(C, M) for C in range(2, 11) for M in range(0, 4)]
    for (C, M), line in zip(cases, planner(["P %d %d" % cm for cm in cases])):
        coarse_at, done_r = [], 0
        for j in range(1, M + 1):
            r = max(done_r + 1, C * j // (M + 1))
            if r >= C:
                break
            coarse_at.append(r)
            done_r = r
        start_of = [0] * C
        for m, at in enumerate(coarse_at):
            for q in range(at, C):
                start_of[q] = m + 1
        a, b = line.split("/")
        assert (ints(a), ints(b)) == (coarse_at, start_of), (C, M)


def stitch_expected(need, refit):
    """The stitch round of sequential_path_chunked after the refits: refit[r] = (m, chunk length, stopped_at)."""
    C = len(need)
    changed, any_, give_up_from = [0] * C, False, -1
    for r in range(1, C):
        changed[r] = 0
        if not need[r]:
            continue
        m, length, stopped_at = refit[r]
        if stopped_at < 0 and m < length:
            if give_up_from < 0 or r < give_up_from:
                give_up_from = r
        elif stopped_at < 0:
            changed[r] = 1
            any_ = True
    if give_up_from >= 0:
        r = 1
        while r < give_up_from:
            if changed[r] and r + 1 < give_up_from:
                give_up_from = r + 1
            r += 1
    nxt = list(need)
    for r in range(1, C):
        nxt[r] = changed[r - 1]
    return changed, any_, give_up_from, nxt


def test_stitch_round_exhaustive_for_four_chunks(planner):
    lens = (3, 5, 8, 13)
    # per needed chunk: met its own chain (early / at its last row), replaced the whole chunk, out of budget
    outcomes = {"met": lambda n: (1, n, 0), "met_last": lambda n: (n, n, n - 1), "whole": lambda n: (n, n, -1),
                "budget": lambda n: (n - 1, n, -1)}
    cases = []
    for mask in itertools.product((0, 1), repeat=3):
        need = [0] + list(mask)
        needed = [r for r in range(1, 4) if need[r]]
        for combo in itertools.product(outcomes, repeat=len(needed)):
            refit = [(0, lens[r], -1) for r in range(4)]
            for r, o in zip(needed, combo):
                refit[r] = outcomes[o](lens[r])
            cases.append((need, refit))
    assert len(cases) == sum(4 ** bin(m).count("1") for m in range(8))
    lines = ["S 4 %s %s" % (" ".join(map(str, need)), " ".join("%d %d %d" % (m, n, st >= 0) for m, n, st in refit))
             for need, refit in cases]
    for (need, refit), line in zip(cases, planner(lines)):
        changed, flags, nxt = (ints(v) for v in line.split("/"))
        want = stitch_expected(need, refit)
        assert (changed, bool(flags[0]), flags[1], nxt) == want, (need, refit)
