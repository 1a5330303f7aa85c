// bessx_kplan.h -- what the chunk chains' driver (bessx_kchunks.cpp: sequential_path_chunked) decides on the host alone:
// where the chunks are cut, which coarse fits run in front of them, what a round of the stitch leaves to the next one.
// Standard library only -- no HIP, no session -- so that tests/test_kchunks_plan.py compiles it on its own.
#ifndef BESSX_KPLAN_H
#define BESSX_KPLAN_H

#include <algorithm>
#include <vector>

namespace bessx {

// chunk r = candidates [bounds[r], bounds[r + 1]): equal lengths.  (Lengths weighted by the level -- a candidate costs
// more the larger its solve -- were measured on configs[1]: 1 + k / 40 ... 1 + k / 400 gave 15.0 ... 12.5 ms per path
// against 12.1 for equal chunks; where the boundaries fall relative to the fills matters more than the balance.)
// The IRLS / Newton families: the later chunks are shorter (their sub-model systems grow with the level: logistic
// 123 ms with lengths weighted 1 + k / 160, 129 ms with equal ones) -- candidate i weighs 1 + seq[i] / wdiv.
// (Chains that share their passes advance in step, one PDAS iteration per shared pass: equal lengths, wdiv = 1e9 --
// with the weights of round 5 the first chunk, the longest, ended 30 % after the others; test hook kchunks_len_div)
inline std::vector<int> chunk_bounds(bool model_is_lm, const int *seq, int ns, int C, double wdiv) {
  std::vector<int> bounds((size_t)C + 1, 0);
  if (model_is_lm) {
    for (int r = 1; r <= C; r++) bounds[r] = (int)((long)ns * r / C);
    return bounds;
  }
  double tot = 0.0;
  std::vector<double> cum((size_t)ns + 1, 0.0);
  for (int i = 0; i < ns; i++) {
    tot += 1.0 + (double)seq[i] / wdiv;
    cum[(size_t)i + 1] = tot;
  }
  for (int r = 1; r < C; r++) {
    const int b = (int)(std::lower_bound(cum.begin(), cum.end(), tot * r / C) - cum.begin());
    bounds[r] = std::min(std::max(b, bounds[r - 1] + 1), ns - (C - r));
  }
  bounds[C] = ns;
  return bounds;
}

// In front of the chunks: at most M coarse fits, at chunk boundaries spread evenly over the path: with more chunks than
// that a chunk starts from the nearest coarse model below it (or cold, in front of the first one) -- its own first fits
// bridge the gap side by side with the other chunks, where a coarse fit per chunk (7 for 8 chunks: + 1.2 ms on
// configs[1]) would run before any of them.
struct CoarsePlan {
  std::vector<int> coarse_at;  // coarse fit m (1-based) ends at the lower boundary of chunk coarse_at[m - 1]
  std::vector<int> start_of;   // chunk r starts from coarse fit start_of[r] (0: cold, or the link's model)
};
inline CoarsePlan coarse_plan(int C, int M) {
  CoarsePlan pl;
  int done_r = 0;
  for (int j = 1; j <= M; j++) {
    const int r = std::max(done_r + 1, (int)((long)C * j / (M + 1)));
    if (r >= C) break;
    pl.coarse_at.push_back(r);
    done_r = r;
  }
  pl.start_of.assign((size_t)C, 0);
  for (size_t m = 0; m < pl.coarse_at.size(); m++)
    for (int q = pl.coarse_at[m]; q < C; q++) pl.start_of[(size_t)q] = (int)m + 1;
  return pl;
}

// One round of the stitch.  The refit of a needed chunk r >= 1 replaced the chunk's first m candidates (of len) and met
// the chunk's own chain there (stopped_at >= 0: the two chains are one from there on) or did not.
struct StitchRefit {
  int m = 0, len = 0;
  bool met = false;
};
struct StitchRound {
  std::vector<char> changed;  // the chunk was replaced as a whole: its last model is a new one
  std::vector<char> need;     // the NEXT round's refits: the chunks behind a changed one
  bool any = false;
  int give_up_from = -1;  // >= 1: the first unsettled chunk, from which the rest is walked as one chain
};
inline StitchRound stitch_round(const std::vector<char> &need, const std::vector<StitchRefit> &refit) {
  const int C = (int)need.size();
  StitchRound d{std::vector<char>((size_t)C, 0), std::vector<char>((size_t)C, 0)};
  for (int r = 1; r < C; r++) {
    if (!need[r]) continue;
    const StitchRefit &t = refit[(size_t)r];
    if (!t.met && t.m < t.len) {
      // out of budget without meeting the chunk's own chain
      if (d.give_up_from < 0 || r < d.give_up_from) d.give_up_from = r;
    } else if (!t.met) {  // the whole (short) chunk was replaced
      d.changed[r] = 1;
      d.any = true;
    }
  }
  if (d.give_up_from >= 0) {
    // a chunk behind one whose last model changed in this round was refitted from the old model: unsettled too
    for (int r = 1; r < d.give_up_from; r++)
      if (d.changed[r] && r + 1 < d.give_up_from) d.give_up_from = r + 1;
  }
  for (int r = 1; r < C; r++) d.need[r] = d.changed[r - 1];
  return d;
}

}  // namespace bessx

#endif  // BESSX_KPLAN_H
