// bessx_kchunks.cpp -- sequential_path (src/path.cpp:25-132) of ONE LM problem as several chunk chains at once.
//
// Candidate k of the path starts from candidate k-1's model (src/path.cpp:60-64): one chain of dependent fits whose
// kernels are single workgroups -- one compute unit of 256 busy between the passes over X that bring new Gram columns.
// The multi-GPU run cuts the chain into chunks and STITCHES them back into the single chain
// (bess_amd.dist.StitchedKPath); here the same is done inside one device, on ONE Gram column cache:
//   1. a coarse warm-start chain over the sparsity levels in front of the chunks (C - 1 fits): it fills the cache with
//      nearly every column the path will ask for (its fills speculate 64 columns wide) and leaves every chunk the model
//      it starts from;
//   2. the C chunks side by side, each on a fit context of its own (stream, host thread, control block, scores, solve
//      work space) that reads the shared cache.  A chunk that needs a column the cache lacks fills it while every
//      other chain stands still between two candidates (the rendezvous below): nobody reads the slot map while it is
//      rewritten;
//   3. the stitch: chunk r re-fits its first candidates warm from chunk r-1's last model until one coincides with its
//      own (same support, coefficients to 1e-9) -- from there on the two chains are the same chain -- and replaces what
//      was walked before; in rounds, until no chunk's last model changed.
// The candidates returned are the single chain's: same supports, iteration counts and criteria
// (tests/test_kchunks_gpu.py; at full size tests/test_fullsize_gpu.py).
#include "bessx_host.h"
#include "bessx_kplan.h"
#include <optional>

namespace bessx {

// The chains' shared passes over X (round 6; the protocol is bessx_sync.h: PassRendezvous).  The chunk chains of the
// streaming forms -- LM with score_mode 1, logistic, Poisson, Cox -- need X^T v (or the Cox score) for a vector of their own
// at every PDAS iteration.  Issued per chain every one of them streams the whole of X (round 5: 153 / 220 / 241 / 251
// passes per path of the four full-size configs, the passes of three or four chains side by side at 0.44-0.65 of the HBM
// roof each).  Here a chain hands its vector set to the owner's next MULTI-CHAIN launch (k_xtv_mc, k_cox_score1p_mc: X is
// loaded once, every active chain's sums are formed from it, bitwise those of a launch of its own) on the PASS STREAM:
// the launch waits for an event every participant records on its own stream (its vectors are ready), every participant's
// stream waits for the event recorded behind the launch.  A pass then serves every chain that is at its score pass --
// the chains fall into step at the passes, and the count of chains is no longer bounded by what a pass per chain costs.
struct SharedPass {
  PassRendezvous rdv;
  bool on = false;     // this path's chains share their passes
  int kind = 0;        // 0: k_xtv_mc, one vector; 1: k_xtv_mc, two vectors (GLM); 2: k_cox_score1p_mc
  int cap = XTV_MC_MAX;
  hipStream_t st = nullptr;
  std::mutex launch_mu;  // one batch's (waits, launch, records) on the pass stream at a time
  hipEvent_t ev_in[XTV_MC_MAX] = {};
  static constexpr int RING = 8;
  hipEvent_t ev_out[RING] = {};
  XtvMc xq = {};
  CoxMc cq = {};
  std::atomic<int> rc{0};  // first error of a batch (reported by the path)
  void fail_with(hipError_t e) {  // (the first error wins)
    int none = 0;
    if (e != hipSuccess) rc.compare_exchange_strong(none, (int)e);
  }
  // statistics: HIP events around every launch on the pass stream, and how many gates were open in it
  bool timing = false;
  std::vector<hipEvent_t> tev;
  size_t tused = 0;
  int *ran = nullptr;  // device, RAN_CAP ints
  static constexpr int RAN_CAP = 8192;
  int launches = 0;
  Owner own;  // the events and `ran`
};

struct KChains {
  std::vector<bessx_session *> ctx;
  // the chains of merged runs of many responses (mc_contexts): apart from the chunk chains' contexts, whose streams have
  // hardware queues of their own; these queue nothing on theirs
  std::vector<bessx_session *> mc_ctx;
  FoldPool pool;
  bool pool_started = false;
  SharedPass sp;
  FillRendezvous rdv;  // the fill rendezvous (bessx_sync.h: built and hammered under ThreadSanitizer, tools/tsan)
  // candidates a chunk chain has stored so far / whether it has ended (read by its predecessor's early stitch)
  std::atomic<int> progress[10];
  std::atomic<int> ended[10];  // 0 running, 1 ended, 2 failed
  // test hook kchunks_log=1: what every chain did when (to stderr at the end of the path)
  bool log_on = false;
  std::mutex log_mu;
  std::chrono::steady_clock::time_point log_t0;
  struct LogRow {
    double ms;
    int chain;
    const char *what;
    int a, b;
  };
  std::vector<LogRow> log;
  // merged launches over the chains (mc_engine): device copies of the chains' descriptions and states, the chunk's
  // levels, the per-candidate records; pinned status block and its sequence number
  McChain *mc_chains = nullptr;
  McState *mc_states = nullptr;
  int *mc_seq = nullptr, *mc_rec_i = nullptr, *mc_rec_A = nullptr;
  double *mc_rec_d = nullptr, *mc_rec_b = nullptr;
  size_t mc_cap_cand = 0, mc_cap_cells = 0, mc_cap_seq = 0;
  unsigned char *mc_status_h = nullptr;
  unsigned long long *mc_flag = nullptr, mc_seq_no = 0;
  // (per chain, mc_cap_chains of each: the union fill's lists beyond 8 and the resume list -- device, pinned staging)
  int mc_cap_chains = 0;
  const int **mc_ulist = nullptr;
  int *mc_ulen = nullptr, *mc_rlist = nullptr;
  unsigned char *mc_stage_h = nullptr;
  Owner chains_own, own;  // what is sized by the number of chains (released when that grows); the rest, kch_slot_w included
};

// between two candidates of a chunk chain: if another chain waits to fill, drain this chain's stream and stand still
void kchains_safe_point(bessx_session *c) {
  KChains *k = c->kch_owner ? c->kch_owner->kch : nullptr;
  if (!k) return;
  k->rdv.safe_point([c] { (void)hipStreamSynchronize(c->st); });
}

// a parked chain asks for the cache: returns 0 when it may fill (every other chain stands still), 1 when another chain
// filled while this one waited (the right is held all the same: look the columns up again), -1 when the run was abandoned
int kchains_fill_begin(bessx_session *c) {
  FillRendezvous &rdv = c->kch_owner->kch->rdv;
  const int waited = rdv.fill_begin([c] { (void)hipStreamSynchronize(c->st); }, c->kch_gen_seen);
  if (waited >= 0) c->kch_gen_seen = rdv.generation();  // (the right is held: no fill ends before this chain's does)
  return waited;
}

void kchains_fill_end(bessx_session *c, bool filled) { c->kch_owner->kch->rdv.fill_end(filled); }

void kchains_log(bessx_session *c, const char *what, int a, int b) {
  bessx_session *o = c->kch_owner ? c->kch_owner : c;
  KChains *k = o->kch;
  if (!k || !k->log_on) return;
  int id = -1;
  for (size_t i = 0; i < k->ctx.size(); i++)
    if (k->ctx[i] == c) id = (int)i;
  const double ms = std::chrono::duration<double>(std::chrono::steady_clock::now() - k->log_t0).count() * 1e3;
  std::lock_guard<std::mutex> lk(k->log_mu);
  k->log.push_back({ms, id, what, a, b});
}

// a chain context has stored its n-th candidate (rows < n of its result arrays are final)
void kchains_progress(bessx_session *c, int n) {
  KChains *k = c->kch_owner ? c->kch_owner->kch : nullptr;
  if (!k || c->kch_index < 0 || c->kch_index >= 10) return;
  if (k->ended[c->kch_index].load(std::memory_order_acquire) != 0) return;  // (a refit on the context of an ended chunk)
  k->progress[c->kch_index].store(n, std::memory_order_release);
}

bool kchains_staged(const bessx_session *c) {
  return c->kch_owner && c->kch_owner->kch && c->kch_owner->kch->rdv.concurrent;  // (set before the round's chains start)
}

unsigned long long kchains_generation(bessx_session *c) { return c->kch_owner->kch->rdv.generation(); }

static void kchains_round(KChains *k, int chains, bool staged = false) { k->rdv.round(chains, staged); }

// ---- shared passes -------------------------------------------------------------------------------------------------
static void sp_free(SharedPass &sp) {
  if (sp.st) ctx_stream_destroy(sp.st);
  sp.own.release();
  sp.st = nullptr;
  sp.ran = nullptr;
  sp.tev.clear();
  for (auto &e : sp.ev_in) e = nullptr;
  for (auto &e : sp.ev_out) e = nullptr;
}

// stream, events and the gate counters of the pass stream; false: not to be had (the chains then keep their own passes)
static bool sp_prepare(bessx_session *s, SharedPass &sp) {
  if (sp.st) return true;
  if (!ctx_stream_create(s->device, &sp.st)) {
    int lo = 0, hi = 0;
    if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess ||
        hipStreamCreateWithPriority(&sp.st, hipStreamNonBlocking, hi) != hipSuccess) {
      (void)hipGetLastError();
      sp.st = nullptr;
      return false;
    }
  }
  bool ok = true;
  for (auto &e : sp.ev_in) ok = ok && sp.own.event(&e, hipEventDisableTiming) == hipSuccess;
  for (auto &e : sp.ev_out) ok = ok && sp.own.event(&e, hipEventDisableTiming) == hipSuccess;
  ok = ok && sp.own.alloc(&sp.ran, SharedPass::RAN_CAP) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    sp_free(sp);
    return false;
  }
  return true;
}

// (under the rendezvous' lock) launch the n requests collected as batch g
static void sp_launch(bessx_session *o, SharedPass &sp, int n, unsigned long long g) {
  std::lock_guard<std::mutex> lk(sp.launch_mu);
  // after an error (a chain's vectors may not be ordered before the batch) nothing is launched any more: the path fails
  // with sp.rc; ev_out is recorded all the same, so that no participant waits for an event that never comes
  const bool dead = sp.rc.load() != 0;
  hipError_t e = hipSuccess;
  for (int i = 0; i < n && e == hipSuccess && !dead; i++) e = hipStreamWaitEvent(sp.st, sp.ev_in[i], 0);
  int *ran = nullptr;
  hipEvent_t ea = nullptr, eb = nullptr;
  if (sp.timing && !dead && sp.launches < SharedPass::RAN_CAP) {
    while (sp.tev.size() < sp.tused + 2) {
      hipEvent_t ev = nullptr;
      if (sp.own.event(&ev) != hipSuccess) break;
      sp.tev.push_back(ev);
    }
    if (sp.tev.size() >= sp.tused + 2) {
      ea = sp.tev[sp.tused];
      eb = sp.tev[sp.tused + 1];
      ran = sp.ran + sp.tused / 2;
      sp.tused += 2;
    }
  }
  if (ea && e == hipSuccess) e = hipEventRecord(ea, sp.st);
  if (e == hipSuccess && !dead) {
    if (sp.kind == 2) {
      sp.cq.nc = n;
      sp.cq.ran = ran;
      e = launch_cox_score1p_mc(o->X, o->ld, o->p, o->U, o->nrb, sp.cq, sp.st);
    } else {
      sp.xq.nc = n;
      sp.xq.ran = ran;
      e = launch_xtv_mc(o->X, o->ld, o->p, o->U, sp.xq, sp.kind == 1, sp.st);
    }
  }
  if (eb && e == hipSuccess) e = hipEventRecord(eb, sp.st);
  if (e == hipSuccess) e = hipEventRecord(sp.ev_out[g % SharedPass::RING], sp.st);
  sp.launches++;
  if (e != hipSuccess) (void)hipGetLastError();
  sp.fail_with(e);
}

bool shared_pass_applies(const bessx_session *c) {
  return c && c->kch_owner && c->kch_owner->kch && c->kch_owner->kch->sp.on && c->kch_sp_member;
}

// The pass over X of slot `slot` of chain context c's fit: its vectors go into the owner's next multi-chain launch.
// Returns when that launch is queued and c's stream is ordered behind it.  v2 / part2: the second accumulator (GLM);
// cox != nullptr: the one-pass Cox score (part = its output planes).
int shared_pass_submit(bessx_session *c, const double *v, const double *v2, double *part, double *part2,
                       const CoxBufs *cox, const FitCtrl *ctrl, int slot) {
  bessx_session *o = c->kch_owner;
  SharedPass &sp = o->kch->sp;
  hipError_t e_in = hipSuccess, e_out = hipSuccess;
  sp.rdv.submit(
      [&](int i) {
        if (cox) {
          CoxMc &q = sp.cq;
          q.TH[i] = cox->TH;
          q.CU[i] = cox->CU;
          q.CV[i] = cox->CV;
          q.C2[i] = cox->C2;
          q.out[i] = part;
          q.ctrl[i] = ctrl;
          q.slot[i] = slot;
        } else {
          XtvMc &q = sp.xq;
          q.v[i] = v;
          q.v2[i] = v2;
          q.part[i] = part;
          q.part2[i] = part2;
          q.ctrl[i] = ctrl;
          q.slot[i] = slot;
        }
        e_in = hipEventRecord(sp.ev_in[i], c->st);  // everything this chain has queued so far: its vectors are ready
        sp.fail_with(e_in);  // (before the batch is launched: sp_launch then launches nothing)
      },
      [&](int n, unsigned long long g) { sp_launch(o, sp, n, g); },
      [&](unsigned long long g) { e_out = hipStreamWaitEvent(c->st, sp.ev_out[g % SharedPass::RING], 0); });
  sp.fail_with(e_out);
  if (const int rc = sp.rc.load()) return fail(BESSX_ERR_HIP, std::string("shared pass over X: ") + hipGetErrorString((hipError_t)rc));
  return 0;
}

// a chain context's thread stops / starts taking part in the shared passes (end of its job; a wait that is not for the
// device).  Leaving while everybody else waits launches their batch.
static void sp_leave(bessx_session *c) {
  if (!c->kch_sp_member) return;
  bessx_session *o = c->kch_owner;
  SharedPass &sp = o->kch->sp;
  c->kch_sp_member = false;
  sp.rdv.leave([&](int n, unsigned long long g) { sp_launch(o, sp, n, g); });
}

static void sp_join(bessx_session *c) {
  SharedPass &sp = c->kch_owner->kch->sp;
  if (!sp.on || c->kch_sp_member) return;
  sp.rdv.join();
  c->kch_sp_member = true;
}

// a round of `members` chain threads starts (before any of them runs)
static void sp_round(KChains *k, const std::vector<bessx_session *> &who) {
  SharedPass &sp = k->sp;
  for (bessx_session *c : k->ctx) c->kch_sp_member = false;
  if (!sp.on) return;
  for (bessx_session *c : who) c->kch_sp_member = true;
  sp.rdv.reset((int)who.size());
}

// after the path (every chain's stream is idle): the launches' times into the session's score-pass statistics
// (whether or not the device answers, the counters start over: nothing carries into the session's next path)
static int sp_collect(bessx_session *s, SharedPass &sp) {
  if (!sp.st) return 0;
  const int nl = (int)(sp.tused / 2);
  auto times = [&]() -> int {
    std::vector<int> ran((size_t)nl, 0);
    HIPX(hipMemcpy(ran.data(), sp.ran, (size_t)nl * sizeof(int), hipMemcpyDeviceToHost));
    for (int i = 0; i < nl; i++) {
      if (ran[(size_t)i] <= 0) continue;  // (every gate closed: the launch fell through)
      float ms = 0.f;
      HIPX(hipEventElapsedTime(&ms, sp.tev[(size_t)2 * i], sp.tev[(size_t)2 * i + 1]));
      s->k1_seconds += (double)ms * 1e-3;
      s->k1_launches += 1;
      s->k1_bytes += 8.0 * (double)s->n * (double)s->p;
      s->sp_chain_slots += ran[(size_t)i];
    }
    return 0;
  };
  int rc = stream_wait_bounded(s, sp.st, "shared pass over X");
  if (rc == 0 && sp.timing && nl > 0) rc = times();
  s->sp_launches += sp.launches;
  s->sp_partial += (long long)sp.rdv.partial;
  sp.rdv.partial = 0;
  sp.tused = 0;
  sp.launches = 0;
  return rc;
}

// The scope of a path's shared-pass round, opened where the chunk chains start: however the driver is left, no context
// stays a member, sp.on is off and the pass stream's launches are collected.  close() is the regular way out and reports
// the round's errors; on a way out that fails already the destructor does the same and keeps the first error's text.
struct SharedPassScope {
  bessx_session *s;
  KChains *k;
  bool open = true;
  SharedPassScope(bessx_session *s_, KChains *k_, int C, bool lm_cov) : s(s_), k(k_) {
    // the chains of the streaming forms share their passes over X (SharedPass above; test hook kchunks_shared_pass=0:
    // a pass per chain, as in round 5)
    SharedPass &sp = k->sp;
    const char *eh = test_hook("kchunks_shared_pass");
    sp.kind = s->model_type == 1 ? 0 : (s->model_type == 4 ? 2 : 1);
    sp.cap = sp.kind == 2 ? COX_MC_MAX : XTV_MC_MAX;
    sp.on = !lm_cov && C >= 2 && C <= sp.cap && (!eh || std::atoi(eh) != 0) &&
            (sp.kind != 2 || s->cox.one_pass) && sp_prepare(s, sp);
    sp.timing = s->timing;
    sp.rc = 0;
    sp.rdv.timeout_s = std::min(0.05, s->wait_deadline_s);
    sp_round(k, std::vector<bessx_session *>(k->ctx.begin(), k->ctx.begin() + C));
  }
  int close() {
    if (!open) return 0;
    open = false;
    for (bessx_session *c : k->ctx) c->kch_sp_member = false;
    k->sp.on = false;
    // (a lost host thread may still be inside a batch: neither the pass stream nor the rendezvous is touched -- what
    // kchains_free leaks on purpose)
    if (k->pool.broken) return 0;
    if (int rc = sp_collect(s, k->sp)) return rc;
    if (const int e = k->sp.rc.load()) return fail(BESSX_ERR_HIP, std::string("shared pass over X: ") + hipGetErrorString((hipError_t)e));
    return 0;
  }
  ~SharedPassScope() {
    const std::string first = g_err;
    if (close() != 0) (void)hipGetLastError();
    g_err = first;
  }
};

static void kchains_leave(KChains *k, bool failed) { k->rdv.leave(failed); }

void kchains_free(bessx_session *s) {
  if (!s || !s->kch) return;
  KChains *k = s->kch;
  if (k->pool_started) k->pool.stop();
  if (s->kch_fill_st) ctx_stream_destroy(s->kch_fill_st);
  s->kch_fill_st = nullptr;
  for (bessx_session *c : k->ctx) ctx_free(c);
  for (bessx_session *c : k->mc_ctx) ctx_free(c);
  // (a broken pool's threads may still touch it and what its owners hold: leaked on purpose)
  if (!k->pool.broken) {
    sp_free(k->sp);
    delete k;
  }
  s->kch = nullptr;
  s->kch_slot_w = nullptr;
}

// how many chunk chains for this path (1 = the single chain)
static int chains_for(const bessx_session *s, int ns, bool link = false, bool link_warm = false) {
  int C = s->kpath_chains;
  if (C == 0 && s->kch_auto_off) return 1;  // (this session's chunks do not merge: see the stitch's budget)
  if (C == 0 && link && s->model_type == 1 && ns < 96) {
    // a link of a longer chain (a rank's chunk of a multi-GPU k-path): shorter, so fewer chains
    C = (ns >= 40 && s->p >= 2048) ? 2 : 1;
    // ... behind lead fits (bessx_path_chain.lead_levels: the link starts warm on a filled cache) short links pay too
    if (link_warm && s->cov_mode && s->p >= 2048) C = ns >= 40 ? 4 : (ns >= 24 ? 3 : (ns >= 16 ? 2 : 1));
  } else if (C == 0 && link && !(s->model_type == 1 && s->cov_mode) && ns < 48) {
    // a short link of a multi-GPU k-path of the families whose every PDAS iteration is a pass over X: with shared passes
    // (round 6) 12-23 levels pay as 2-3 chains -- rank 4 of 8 of configs[4] (levels 77..95, cold) 208 / 186 / 154 ms
    // with 1 / 2 / 3 chains (tools/cox_link_probe.py); every rank of 8: slowest 358 -> 320 ms.  Longer links do not
    // (the 37-level links of 4 ranks: 267 / 178 / 277 ms either way, and the last one -- levels 114..150, beyond the
    // planted support, where cold chunks wander and the stitch gives up -- 571 -> 740 ms): one chain from 24 levels on
    const char *esh = test_hook("kchunks_shared_pass");
    const bool big = (double)s->n * s->p >= 1e8 && (!esh || std::atoi(esh) != 0) && ctx_streams_own_queue(s->device);
    C = (big && ns < 24) ? (ns >= 18 ? 3 : (ns >= 12 ? 2 : 1)) : 1;
  } else if (C == 0) {
    // automatic: long paths on wide designs.  How many chains pay depends on how many hardware queues the HIP runtime
    // gives the process' streams (GPU_MAX_HW_QUEUES, default 4; read when the runtime starts): configs[1], 18.6 ms as
    // one chain -- 4 queues: 2 chains 16.2 ms, 3 and more lose (21.2 / 19.5 ms: streams share queues and wait for each
    // other); 8 queues: 3 chains 14.9 ms, 4 chains 12.7 ms, 6 chains 16.8 ms (tools/kchunks_bench.py)
    // Round 5: the chains' streams are created with a hardware queue of their own, outside that pool
    // (ctx_stream_create), so the count no longer depends on the variable; where such streams cannot be had the old
    // rule stands.
    const char *q = std::getenv("GPU_MAX_HW_QUEUES");
    const int queues = ctx_streams_own_queue(s->device) ? 8 : (q ? std::atoi(q) : 4);
    if (s->model_type == 1 && s->cov_mode)
      C = (ns >= 96 && s->p >= 2048) ? (queues >= 8 ? 4 : 2) : 1;
    else if (s->model_type == 1)
      // round 5: the STREAMING form of the LM score pass as chunk chains, like the IRLS / Newton families -- every PDAS
      // iteration is a pass over X, and one chain's selection, Gram panel, solve and residual run beside another's pass
      // (tools/streaming_chains_bench.py, configs[1]: 190.1 ms as one chain, 168.7 / 173.5 / 162.3 ms with 2 / 3 / 4)
    {
      C = (ns >= 48 && (double)s->n * s->p >= 1e8) ? (queues >= 8 ? 4 : 2) : 1;
      // round 6, shared passes + the light confirming iteration: 8 chains share a pass at 0.75 ms (4: 0.71) -- configs[1]
      // 79 ms per path with 8 chains, 87 with 4 (tools/shared_pass_sweep.py)
      const char *esh = test_hook("kchunks_shared_pass");
      if (C == 4 && (!esh || std::atoi(esh) != 0) && ns >= 128) C = 8;
    } else {
      // logistic / Poisson / Cox: one chain's IRLS or Newton steps (small kernels) run beside another's pass over X
      // (tools/glm_two_chains_probe.py: logistic at full size 155 -> 120 ms with 3 chains, Cox 1.86 -> 1.60 s)
      C = (ns >= 48 && (double)s->n * s->p >= 1e8) ? (queues >= 8 ? 3 : 2) : 1;
      // round 6, shared passes (a pass serves every chain that is at its score pass; tools/shared_pass_sweep.py, full
      // size): logistic 3 / 4 / 6 / 8 chains 85-90 / 90 / 87.5 / 83 ms, Poisson 92 / 90 / 82 / 84 ms per path -- 6; Cox
      // 2 / 3 / 4 chains 1.21 / 1.04 / 1.11 s -- 3
      const char *esh = test_hook("kchunks_shared_pass");
      if (C == 3 && (!esh || std::atoi(esh) != 0) && s->model_type != 4 && ns >= 96) C = 6;
    }
  }
  // (at least 8 candidates per chain; 6 for the families whose every iteration is a pass over X: a short link of a
  // multi-GPU k-path there still pays to share its passes)
  const bool streaming = !(s->model_type == 1 && s->cov_mode);
  return std::max(1, std::min(std::min(C, 8), ns / (streaming ? 6 : 8)));
}

bool kchunks_apply(const bessx_session *s, const int *seq, int ns, int nl, int is_cv, const bessx_path_chain *chain) {
  if (!s || s->kch_owner || s->parent || is_cv || nl != 1) return false;
  // a link of a longer chain (bessx_session_sequential_path_chain) qualifies when it only starts from a given model
  // -- the stitch refits, which stop at the first candidate equal to the caller's, are short and stay one chain
  if (chain && (chain->stop_support || chain->init_len > s->cap)) return false;
  if (s->grouped || !s->warm_start || s->trace.on || s->cv_shared || !s->publish || s->fill_hook) return false;
  if (s->model_type == 1 && s->cov_mode) {
    if (!s->chain) return false;
    if (s->cov_C < (s->p + 31) / 32 * 32 + COV_R) return false;  // the cache must hold every column: it is never started over
  } else if (s->K > 0) {
    return false;  // (sessions with CV folds keep per-row-set state the chain contexts do not own)
  }
  if (chains_for(s, ns, chain != nullptr, chain && chain->init_len > 0 && chain->keep_caches) < 2) return false;
  int top = 0;
  for (int i = 0; i < ns; i++) {
    if (seq[i] < 1 || (i && seq[i] <= seq[i - 1])) return false;  // ascending levels: every chunk continues its predecessor
    top = std::max(top, seq[i]);
  }
  if (top > 254 || top > s->cap) return false;  // (the register-resident solvers)
  return !(s->model_type == 1 && s->cov_mode) || top + COV_R + s->cov_spec <= s->cov_C;
}

namespace {

struct ChunkRun {  // one chunk's candidates, as sequential_path stores them
  int lo = 0, hi = 0, width = 0;
  std::vector<int> T0, iters, support;
  std::vector<double> lam, loss, ic, coef0, beta;
  bessx_path_result res = {};
  bessx_path_chain chain = {};
  std::vector<int> init_idx, last_idx;
  std::vector<double> init_val, last_val;
  double last_coef0 = 0.0;
  int last_len = 0;
  int rc = 0;
  std::string err;  // (the message of a failure on a host thread: bessx_last_error is per thread)

  void shape(int lo_, int hi_, int width_) {
    lo = lo_;
    hi = hi_;
    width = width_;
    const size_t m = (size_t)std::max(1, hi - lo);
    T0.assign(m, 0);
    iters.assign(m, 0);
    lam.assign(m, 0.0);
    loss.assign(m, 0.0);
    ic.assign(m, 0.0);
    coef0.assign(m, 0.0);
    support.assign(m * width, -1);
    beta.assign(m * width, 0.0);
    last_idx.assign((size_t)width, 0);
    last_val.assign((size_t)width, 0.0);
  }
  // The chain link this run walks, into its own arrays: from the model (idx, val, c0) -- copied in: the link points at
  // nothing its ChunkRun does not own --, the caches kept; with `stop`: until a candidate equals one of stop's first
  // stop_rows rows (same support, coefficients to 1e-9).  The last model goes to last_idx / last_val.
  void link(const int *idx, const double *val, int len, double c0, const ChunkRun *stop = nullptr, int stop_rows = 0) {
    res = bessx_path_result();
    res.capacity = hi - lo;
    res.cand_T0 = T0.data();
    res.cand_lambda = lam.data();
    res.cand_iters = iters.data();
    res.cand_train_loss = loss.data();
    res.cand_ic = ic.data();
    res.cand_coef0 = coef0.data();
    res.cand_support = support.data();
    res.cand_beta = beta.data();
    res.max_T0 = width;
    init_idx.assign(idx, idx + len);
    init_val.assign(val, val + len);
    chain = bessx_path_chain();
    chain.init_idx = init_idx.data();
    chain.init_val = init_val.data();
    chain.init_len = len;
    chain.init_coef0 = c0;
    chain.keep_caches = 1;
    if (stop) {
      chain.stop_support = stop->support.data();
      chain.stop_beta = stop->beta.data();
      chain.stop_rows = stop_rows;
      chain.stop_row_len = width;
      chain.stop_rtol = 1e-9;
    }
    chain.last_idx = last_idx.data();
    chain.last_val = last_val.data();
    chain.last_cap = width;
  }
  void link_behind(const ChunkRun &pred, const ChunkRun *stop = nullptr, int stop_rows = 0) {  // from pred's last model
    link(pred.last_idx.data(), pred.last_val.data(), pred.last_len, pred.last_coef0, stop, stop_rows);
  }
};

// the context's own state starts over (the shared cache stays as it is); keep_model: except the model its last fit left
// on the device -- the early stitch continues from exactly that model, without uploading it again
int context_begin(bessx_session *c, bool keep_model = false) {
  if (int rc = settle_device_chain(c)) return rc;
  if (!keep_model) {
    for (auto &q : c->cache) q.valid = q.model_only = false;
    c->dev_state_rs = -1;
  }
  c->trace.clear();
  c->metric_depth = 0;
  c->n_fits = 0;
  c->n_iters = 0;
  return 0;
}

}  // namespace

// every chain context's stream idle (after a failed run a context may still have launches queued)
void kchains_quiesce(bessx_session *s) {
  if (!s || !s->kch) return;
  for (bessx_session *c : s->kch->ctx) (void)hipStreamSynchronize(c->st);
  for (bessx_session *c : s->kch->mc_ctx) (void)hipStreamSynchronize(c->st);
}

void kchains_contexts(const bessx_session *s, std::vector<bessx_session *> *out) {
  out->clear();
  if (!s || !s->kch) return;
  out->insert(out->end(), s->kch->ctx.begin(), s->kch->ctx.end());
  out->insert(out->end(), s->kch->mc_ctx.begin(), s->kch->mc_ctx.end());
}

// Contexts and host threads for the path's chains.  Non-zero when they cannot be had (no memory for the contexts, host
// threads lost in an earlier call): the caller then runs the path as one chain -- slower, same result.
int kchunks_prepare(bessx_session *s, int ns, bool link, bool link_warm) {
  const int C = chains_for(s, ns, link, link_warm);
  if (hipSetDevice(s->device) != hipSuccess) return 1;
  if (!s->kch) s->kch = new KChains();
  KChains *k = s->kch;
  if (k->pool.broken) return 1;
  k->rdv.deadline_s = s->wait_deadline_s;
  while ((int)k->ctx.size() < C) {
    bessx_session *c = nullptr;
    if (chain_ctx_create(s, &c) != 0) {
      (void)hipGetLastError();
      return 1;
    }
    c->kch_index = (int)k->ctx.size();
    k->ctx.push_back(c);
  }
  if (!k->pool_started || (int)k->pool.th.size() < C - 1) {  // one host thread per chain; the caller is one of them
    if (k->pool_started) k->pool.stop();
    k->pool.quit = false;  // (a pool started again: no job of the previous threads' numbering is left to run)
    k->pool.ticket = 0;
    k->pool.ticket_hint.store(0);
    k->pool.job = nullptr;
    {
      const int dev = s->device;
      k->pool.start(C - 1, [dev] { (void)hipSetDevice(dev); });
    }
    k->pool_started = true;
  }
  return 0;
}

// ----------------------------------------------------------------------------------------------------------------
// Merged launches on ONE stream (bessx_dev.h: McChain): the paths of many responses (bessx_multi.cpp), run by mc_engine.
// ----------------------------------------------------------------------------------------------------------------
bool mc_engine_applies(const bessx_session *s) {
  return s->model_type == 1 && s->cov_mode && s->fuse && s->fuse_sel && s->cov_cg && s->cg_by_rows;
}

namespace {

struct McHostStatus {
  McState st;
  FitCtrl ctrl;
};
static_assert(sizeof(McHostStatus) == 192, "192 bytes per chain in the pinned status block");

int mc_wait(bessx_session *s, KChains *k, unsigned long long want) {
  volatile unsigned long long *flag = k->mc_flag;
  std::chrono::steady_clock::time_point t0;
  bool timed = false;
  for (unsigned spins = 1;; spins++) {
    if (*flag >= want) break;
    if ((spins & 0x3fff) == 0) {
      const auto now = std::chrono::steady_clock::now();
      if (!timed) {
        t0 = now;
        timed = true;
      } else if (std::chrono::duration<double>(now - t0).count() > s->wait_deadline_s) {
        return fail(BESSX_ERR_HIP, "chunk chains (merged launches): no status block from the device within " +
                                       std::to_string(s->wait_deadline_s) + " s (BESSX_WAIT_TIMEOUT_S)");
      }
    }
#if defined(__x86_64__)
    __builtin_ia32_pause();
#endif
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  return 0;
}

}  // namespace

// |y - X beta|^2 of a model by one pass over its columns (what algorithm_fit does when the solve's loss terms cancel)
int mc_sse_by_residual(bessx_session *c, hipStream_t st, const int *idx, const double *val, int T0, double coef0, double *out) {
  int *st_idx = reinterpret_cast<int *>(c->stage_h);
  double *st_val = reinterpret_cast<double *>(c->stage_h + (size_t)c->capA * sizeof(int));
  for (int i = 0; i < T0; i++) {
    st_idx[i] = idx[i];
    st_val[i] = val[i];
  }
  HIPX(hipMemcpyAsync(c->init_idx_d, st_idx, T0 * sizeof(int), hipMemcpyHostToDevice, st));
  HIPX(hipMemcpyAsync(c->init_val_d, st_val, T0 * sizeof(double), hipMemcpyHostToDevice, st));
  HIPX(launch_resid_lm(c->X, c->ld, c->n, c->y, c->mask[0], c->ctrl, 0, c->init_idx_d, c->init_val_d, c->tmpv, c->sse, st, 3,
                       T0, coef0));
  std::vector<double> part((size_t)2 * c->n_sse_blk);
  HIPX(hipMemcpyAsync(part.data(), c->sse, part.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPX(hipStreamSynchronize(st));
  double tr = 0.0;
  for (int b = 0; b < c->n_sse_blk; b++) tr += part[2 * b];
  *out = tr;
  return 0;
}

// ---- the merged-launch core (bessx_host.h: McJob): one chain = a chunk of one response's path or the whole path of one
// response.  Buffers sized by the number of chains, every chain's first fit started, rounds of (score pass, selection +
// solve) pairs, ONE union fill per round for every parked chain, then every chain's records read back.
int mc_engine(bessx_session *s, const int *seq, int ns, std::vector<McJob> &jobs, int nrec, double lambda, int width,
              McRecords &rec, std::vector<int> &takeover, long long *fills) {
  KChains *k = s->kch;
  const int C = (int)jobs.size();
  if (!k || C < 1) return fail(BESSX_ERR_ARG, "merged chains: nothing to run");
  const int p = s->p;
  hipStream_t st = s->st;
  // ---- buffers
  if (C > k->mc_cap_chains) {
    k->chains_own.release();
    k->mc_cap_chains = 0;
    const int cap = std::max(C, 8);
    HIPX(k->chains_own.alloc(&k->mc_chains, (size_t)cap));
    HIPX(k->chains_own.alloc(&k->mc_states, (size_t)cap));
    HIPX(k->chains_own.pinned(&k->mc_status_h, (size_t)cap * sizeof(McHostStatus)));
    HIPX(k->chains_own.alloc(&k->mc_ulist, (size_t)cap));
    HIPX(k->chains_own.alloc(&k->mc_ulen, (size_t)cap));
    HIPX(k->chains_own.alloc(&k->mc_rlist, (size_t)cap));
    HIPX(k->chains_own.pinned(&k->mc_stage_h, (size_t)cap * (sizeof(const int *) + 2 * sizeof(int))));
    if (!k->mc_flag) {
      HIPX(k->own.pinned(&k->mc_flag, 128 / sizeof(unsigned long long)));
      k->mc_flag[0] = 0ull;
      k->mc_seq_no = 0;
    }
    k->mc_cap_chains = cap;
  }
  if ((size_t)ns > k->mc_cap_seq) {
    k->mc_cap_seq = 0;
    HIPX(k->own.regrow(&k->mc_seq, (size_t)ns));
    k->mc_cap_seq = (size_t)ns;
  }
  if ((size_t)nrec > k->mc_cap_cand || (size_t)nrec * width > k->mc_cap_cells) {
    k->mc_cap_cand = k->mc_cap_cells = 0;
    for (void *q : {(void *)k->mc_rec_i, (void *)k->mc_rec_d, (void *)k->mc_rec_A, (void *)k->mc_rec_b}) k->own.release_one(q);
    k->mc_rec_i = k->mc_rec_A = nullptr;
    k->mc_rec_d = k->mc_rec_b = nullptr;
    HIPX(k->own.alloc(&k->mc_rec_i, (size_t)nrec * MC_REC_I));
    HIPX(k->own.alloc(&k->mc_rec_d, (size_t)nrec * MC_REC_D));
    HIPX(k->own.alloc(&k->mc_rec_A, (size_t)nrec * width));
    HIPX(k->own.alloc(&k->mc_rec_b, (size_t)nrec * width));
    k->mc_cap_cand = (size_t)nrec;
    k->mc_cap_cells = (size_t)nrec * width;
  }
  if (!s->fill_ctrl) {
    HIPX(s->cv_own.zeros(&s->fill_ctrl, 1));
    HIPX(s->cv_own.pinned(&s->fill_ctrl_h, 1));
  }
  HIPX(hipMemcpyAsync(k->mc_seq, seq, (size_t)ns * sizeof(int), hipMemcpyHostToDevice, st));
  HIPX(hipMemsetAsync(k->mc_rec_i, 0, (size_t)nrec * MC_REC_I * sizeof(int), st));
  // ---- the chains: their contexts' buffers, the start of their first fit
  std::vector<McChain> hc((size_t)C);
  std::vector<McState> hs((size_t)C);
  for (int r = 0; r < C; r++) {
    McJob &j = jobs[(size_t)r];
    bessx_session *c = j.c;
    if (int rc = context_begin(c)) return rc;
    c->timing = s->timing;
    const int lo = j.lo, ncand = j.ncand, k_init = j.init_idx ? (int)j.init_idx->size() : 0;
    if (ncand < 1 || k_init > c->cap || lo + ncand > ns || j.rec0 + ncand > nrec)
      return fail(BESSX_ERR_ARG, "merged chains: bad chain");
    bessx_session::CovCache &cv = c->cov[0];
    int *st_idx = reinterpret_cast<int *>(c->stage_h);
    double *st_val = reinterpret_cast<double *>(c->stage_h + (size_t)c->capA * sizeof(int));
    for (int i = 0; i < k_init; i++) {
      st_idx[i] = (*j.init_idx)[(size_t)i];
      st_val[i] = (*j.init_val)[(size_t)i];
    }
    if (k_init) {
      HIPX(hipMemcpyAsync(c->init_idx_d, st_idx, k_init * sizeof(int), hipMemcpyHostToDevice, st));
      HIPX(hipMemcpyAsync(c->init_val_d, st_val, k_init * sizeof(double), hipMemcpyHostToDevice, st));
    }
    HIPX(launch_fit_begin(c->ctrl, seq[lo], k_init, c->init_idx_d, c->init_val_d, j.init_coef0, c->A_cur, c->b_cur,
                          c->beta_dense, p, c->hist, st, c->inA));
    McChain &m = hc[(size_t)r];
    m = McChain();
    m.state = k->mc_states + r;
    m.seq = k->mc_seq + lo;
    m.width = width;
    m.max_iter = c->max_iter;
    m.p = p;
    m.G = cv.G;
    m.xty = j.xty ? j.xty : c->xty[0];
    m.xtx = c->xtx[0];
    m.n_t = (double)c->n_train[0];
    m.lambda = lambda;
    m.always = c->always;
    m.d_out = c->part_rs[0];
    m.bd = c->bd;
    m.bmm = c->cov_bmm;
    TopkNeed nd = {cov_speculates(c) ? c->bd : nullptr, c->bd2, p, cov_C_dev(c), cv.slot_of, cv.meta, c->cov_fcols,
                   c->ctrl, c->A_cur, c->cov_bmm, (p + 31) / 32, c->inA, 0, 0};
    nd.cm_A_cur = c->A_cur;
    nd.cm_b_cur = c->b_cur;
    nd.cm_beta_dense = c->beta_dense;
    nd.cm_hist = c->hist;
    nd.cm_hist_beta = c->hist_beta;
    nd.cm_hist_coef0 = c->hist_coef0;
    nd.cm_hist_stride = c->hist_stride;
    nd.cm_inA = c->inA;
    nd.commit_on = 1;
    nd.no_restart = 1;
    m.nd = nd;
    m.nd1 = nd;
    m.nd1.inc1 = 1;
    m.nd1.bmm_fresh = 1;
    m.fz = cov_fuse_args(c, 0, seq[lo], false, nullptr);
    m.A_new = c->A_new;
    m.sol = c->sol;
    m.tol = c->cg_tol;
    m.maxit = 64;
    m.rec_i = k->mc_rec_i + (size_t)j.rec0 * MC_REC_I;
    m.rec_d = k->mc_rec_d + (size_t)j.rec0 * MC_REC_D;
    m.rec_A = k->mc_rec_A + (size_t)j.rec0 * width;
    m.rec_b = k->mc_rec_b + (size_t)j.rec0 * width;
    McState &z = hs[(size_t)r];
    z = McState();
    z.ncand = ncand;
    z.need_d = 1;
    c->dev_state_rs = -1;
  }
  HIPX(hipMemcpyAsync(k->mc_chains, hc.data(), (size_t)C * sizeof(McChain), hipMemcpyHostToDevice, st));
  HIPX(hipMemcpyAsync(k->mc_states, hs.data(), (size_t)C * sizeof(McState), hipMemcpyHostToDevice, st));
  HIPX(hipStreamSynchronize(st));  // (hc / hs / the staging buffers are the host's again)
  // ---- rounds: a batch of (score pass, selection + solve) pairs, then every chain's state
  int longest = 0;
  for (const McJob &j : jobs) longest = std::max(longest, j.ncand);
  // Batches of 8 pairs: a chain that parks on a missing column waits for the end of its batch before the host sees it
  // (queueing the whole chunk ahead -- about one pair per candidate -- left a parked chain idle for up to 2.6 ms on
  // configs[1]); the read-back between two batches costs the device ~25 us of 500.
  int batch = 8;
  const McHostStatus *hstat = reinterpret_cast<const McHostStatus *>(k->mc_status_h);
  takeover.assign((size_t)C, 0);
  const int **stage_lists = reinterpret_cast<const int **>(k->mc_stage_h);
  int *stage_len = reinterpret_cast<int *>(k->mc_stage_h + (size_t)k->mc_cap_chains * sizeof(const int *));
  int *stage_resume = stage_len + k->mc_cap_chains;
  for (int round = 0;; round++) {
    if (round > 64 + longest) return fail(BESSX_ERR_NUMERIC, "merged chains: the chains do not end");
    for (int b = 0; b < batch; b++) {
      HIPX(launch_mc_cov_d(k->mc_chains, C, p, st));
      HIPX(launch_mc_sel_cgr(k->mc_chains, C, p, st));
    }
    const unsigned long long want = ++k->mc_seq_no;
    HIPX(launch_mc_status(k->mc_chains, C, k->mc_status_h, k->mc_flag, want, st));
    if (int rc = mc_wait(s, k, want)) return rc;
    bool all = true;
    std::vector<int> parked;
    for (int r = 0; r < C; r++) {
      const McHostStatus &h = hstat[r];
      if (h.st.finished == 1) continue;
      if (h.st.finished == 2) {
        takeover[(size_t)r] = 1;
        continue;
      }
      if (h.st.parked == 1) {
        parked.push_back(r);
        all = false;
      } else if (h.st.parked) {  // a tie, a solve for the Cholesky kernel, a full cache: the proven path finishes this chain
        HIPX(launch_mc_stop(k->mc_chains, r, st));
        takeover[(size_t)r] = 1;
      } else {
        all = false;
      }
    }
    if (!parked.empty()) {
      // ONE fill for every chain parked on missing columns; nobody else runs (one stream): fold_fits_side_by_side's rule
      CovUnion u = {};
      bessx_session *spec_src = nullptr;
      int ub = 0;
      for (int r : parked) {
        bessx_session *c = jobs[(size_t)r].c;
        if (u.nf < 8) {
          u.list[u.nf] = c->A_new;
          u.len[u.nf++] = hstat[r].ctrl.T0;
        } else {  // (beyond 8 sets: device arrays of lists, listed after the fixed ones)
          stage_lists[u.dn] = c->A_new;
          stage_len[u.dn++] = hstat[r].ctrl.T0;
        }
        ub += hstat[r].ctrl.cov_nmiss;
        if (!spec_src && cov_speculates(c)) spec_src = c;
      }
      if (u.dn > 0) {
        HIPX(hipMemcpyAsync(k->mc_ulist, stage_lists, (size_t)u.dn * sizeof(const int *), hipMemcpyHostToDevice, st));
        HIPX(hipMemcpyAsync(k->mc_ulen, stage_len, (size_t)u.dn * sizeof(int), hipMemcpyHostToDevice, st));
        u.dlist = k->mc_ulist;
        u.dlen = k->mc_ulen;
      }
      if (spec_src)
        HIPX(launch_topk(spec_src->bd2, p, s->cov_spec, spec_src->cov_extras, spec_src->cand, nullptr, 0, st));
      HIPX(launch_cov_fill_union(u, 0, spec_src ? spec_src->cov_extras : nullptr, spec_src ? spec_src->bd2 : nullptr,
                                 s->cov_spec, s->cov_spec / 2, s->cov[0].slot_of, s->cov[0].meta, p, s->cov_fcols,
                                 s->fill_ctrl, st));
      HIPX(hipMemcpyAsync(s->fill_ctrl_h, s->fill_ctrl, sizeof(FitCtrl), hipMemcpyDeviceToHost, st));
      HIPX(hipStreamSynchronize(st));
      s->cov_panel_groups += s->fill_ctrl_h->cov_groups - s->fill_groups_seen;
      s->fill_groups_seen = s->fill_ctrl_h->cov_groups;
      const int ngroups = s->fill_ctrl_h->cov_nfill / COV_R;
      if (ngroups > (ub + s->cov_spec + 2 * COV_R - 1) / COV_R)
        return fail(BESSX_ERR_NUMERIC, "internal error: union fill list longer than its bound (merged chains)");
      if (int rc = enqueue_cov_fill(s, 0, ngroups, 1, s->fill_ctrl)) return rc;
      if (s->timing) {
        HIPX(hipStreamSynchronize(st));
        if (int rc = cov_collect(s, s->fill_ctrl_h->cov_nfill)) return rc;
      }
      for (size_t i = 0; i < parked.size(); i++) stage_resume[i] = parked[i];
      HIPX(hipMemcpyAsync(k->mc_rlist, stage_resume, parked.size() * sizeof(int), hipMemcpyHostToDevice, st));
      HIPX(launch_mc_resume_list(k->mc_chains, k->mc_rlist, (int)parked.size(), st));
      if (fills) (*fills)++;
    }
    if (all) break;
  }
  // ---- the records
  rec.i.assign((size_t)nrec * MC_REC_I, 0);
  rec.A.assign((size_t)nrec * width, 0);
  rec.d.assign((size_t)nrec * MC_REC_D, 0.0);
  rec.b.assign((size_t)nrec * width, 0.0);
  HIPX(hipMemcpyAsync(rec.i.data(), k->mc_rec_i, rec.i.size() * sizeof(int), hipMemcpyDeviceToHost, st));
  HIPX(hipMemcpyAsync(rec.d.data(), k->mc_rec_d, rec.d.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPX(hipMemcpyAsync(rec.A.data(), k->mc_rec_A, rec.A.size() * sizeof(int), hipMemcpyDeviceToHost, st));
  HIPX(hipMemcpyAsync(rec.b.data(), k->mc_rec_b, rec.b.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPX(hipStreamSynchronize(st));
  for (const McJob &j : jobs) {
    for (auto &cc : j.c->cache) cc.valid = cc.model_only = false;  // (the device state of the context is the engine's, not a fit's of its own)
    j.c->dev_state_rs = -1;
  }
  return 0;
}

int mc_contexts(bessx_session *s, int n) {
  if (hipSetDevice(s->device) != hipSuccess) return fail(BESSX_ERR_HIP, "merged chains: device");
  if (!s->kch) s->kch = new KChains();
  KChains *k = s->kch;
  while ((int)k->mc_ctx.size() < n) {
    bessx_session *c = nullptr;
    // (ordinary streams: the merged run queues everything on the session's own)
    if (int rc = chain_ctx_create(s, &c, false)) {
      (void)hipGetLastError();
      return rc;
    }
    c->kch_index = -1;
    k->mc_ctx.push_back(c);
  }
  return 0;
}

bessx_session *mc_context(bessx_session *s, int i) { return s->kch->mc_ctx[(size_t)i]; }

namespace {

using Clock = std::chrono::steady_clock;
double secs(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double>(b - a).count(); }

struct StartModel {
  SparseVec b;
  double c0 = 0.0;
};

// One chunked path: what the phases of sequential_path_chunked (below, in the order they run) hand on to each other.
struct ChunkPath {
  bessx_session *s;
  KChains *k;
  const int *seq;
  int ns;
  double lambda;
  int ic_type, C, width;
  bool lm_cov;
  std::vector<int> bounds;        // plan: chunk r = candidates [bounds[r], bounds[r + 1])
  CoarsePlan coarse;              // plan
  bool staged = false;            // fill_stream
  std::vector<StartModel> start;  // coarse_chain: the model chunk r starts from (none: cold)
  std::vector<ChunkRun> run;      // chunk_round; candidates replaced by stitch_rounds, the end by give_up_tail
  bool early_on = false;          // chunk_round -> stitch_rounds: the refits of round 1 that are there already
  std::vector<ChunkRun> early_st;
  std::vector<char> early_ok;
  long long refits = 0, iters_path = 0;
  int give_up_from = -1;  // stitch_rounds -> give_up_tail
  Clock::time_point t_begin, t_coarse, t_chunks;

  void plan() {
    const char *esh = test_hook("kchunks_shared_pass");
    double wdiv = (!esh || std::atoi(esh) != 0) ? 1e9 : 160.0;
    if (const char *ew = test_hook("kchunks_len_div")) wdiv = std::max(1.0, std::atof(ew));
    bounds = chunk_bounds(s->model_type == 1, seq, ns, C, wdiv);
    // The coarse chain.  (LM only: it is what fills the shared cache.  The other families keep no cache: their chunks start
    // cold, side by side -- a restricted fit is cold-started anyway, only the active set is warm -- and are stitched)
    // At most COARSE_MAX fits (coarse_plan).  Starting points only: the stitch makes the path the single chain's.
    constexpr int COARSE_MAX = 3;
    int M = lm_cov ? std::min(C - 1, COARSE_MAX) : 0;  // (no cache to fill otherwise)
    if (const char *ev = test_hook("kchunks_coarse")) M = std::max(0, std::min(M, std::atoi(ev)));  // (0: every chunk starts cold)
    coarse = coarse_plan(C, M);
  }

  // Staged fills (bessx_sync.h: FillRendezvous, concurrent rounds; test hook kchunks_staged=0/1): a chain's fill writes
  // slots no other chain can see until its last launch publishes them, so nobody stands still for a fill.
  void fill_stream() {
    if (lm_cov) {
      const char *ev = test_hook("kchunks_staged");
      staged = !ev || std::atoi(ev) != 0;  // (default; 0: round 4's rendezvous -- every chain stands still for a fill)
    }
    if (staged && !s->kch_slot_w && k->own.alloc(&s->kch_slot_w, (size_t)s->p) != hipSuccess) {
      (void)hipGetLastError();
      staged = false;
    }
    if (!staged || s->kch_fill_st || s->kch_fill_tried) return;
    s->kch_fill_tried = true;  // (decided once per session: no unit to leave out, or no such stream to be had)
    // the fills' stream: every compute unit but a few (test hook kchunks_reserve=count[:stride of the mask bits]; 0: the
    // fills run on the filling chain's own stream)
    // k_cov_panel_dp runs ONE workgroup per compute unit: the units left out must be ones its rounds of workgroups
    // leave idle anyway (configs[1]: 237 workgroups, one round), or a pass on the fill stream would take a round more
    hipDeviceProp_t prop;
    const int cus = hipGetDeviceProperties(&prop, s->device) == hipSuccess ? prop.multiProcessorCount : 0;
    // (the most units that can go without a round more: rounds = ceil(blocks / units) must stay what it is)
    const int blocks = s->cov_panel_blocks;
    const int rounds = (cus > 0 && blocks > 0) ? (blocks + cus - 1) / cus : 0;
    const int idle = rounds > 0 ? cus - (blocks + rounds - 1) / rounds : 0;
    int leave = idle >= 4 ? std::min(16, idle) : 0, stride = 1;
    if (const char *er = test_hook("kchunks_reserve")) {
      leave = std::max(0, std::atoi(er));
      if (const char *c2 = std::strchr(er, ':')) stride = std::max(1, std::atoi(c2 + 1));
    }
    if (leave > 0 && !ctx_stream_create(s->device, &s->kch_fill_st, leave, stride)) s->kch_fill_st = nullptr;
  }

  // ---- 1. the coarse chain on the session's own state (the caller has just started the caches over)
  int coarse_chain(bessx_path_chain *link) {
    t_begin = Clock::now();
    const char *el = test_hook("kchunks_log");
    k->log_on = el && std::atoi(el) != 0;
    k->log_t0 = t_begin;
    k->log.clear();
    run = std::vector<ChunkRun>((size_t)C);
    start.assign((size_t)C, StartModel());
    if (link) {  // the model the whole link starts from: chunk 0's start, and the coarse chain's
      for (int i = 0; i < link->init_len; i++) {
        if (link->init_idx[i] < 0 || link->init_idx[i] >= s->p) return fail(BESSX_ERR_ARG, "chain: init index out of range");
        start[0].b.idx.push_back(link->init_idx[i]);
        start[0].b.val.push_back(link->init_val[i]);
      }
      start[0].c0 = link->init_coef0;
      link->stopped_at = -1;
    }
    s->hint.on = false;
    StartModel at = start[0];
    for (size_t m = 0; m < coarse.coarse_at.size(); m++) {
      if (int rc = run_fit(s, seq[bounds[(size_t)coarse.coarse_at[m]] - 1], lambda, at.b, at.c0)) return rc;
      at = {s->beta, s->coef0};
      for (int r = 0; r < C; r++)
        if (coarse.start_of[(size_t)r] == (int)m + 1) start[(size_t)r] = at;
    }
    if (int rc = settle_device_chain(s)) return rc;
    HIPX(hipStreamSynchronize(s->st));  // the cache is complete before any chunk chain reads it
    t_coarse = Clock::now();
    return 0;
  }

  // The writer's slot map is a copy of the readers' whenever a round of chains starts (no fill is in flight between two
  // rounds; what ran in between -- the coarse chain -- filled through the readers' map)
  int writer_map_in_step() {
    if (!staged) return 0;
    HIPX(hipMemcpyAsync(s->kch_slot_w, s->cov[0].slot_of, (size_t)s->p * sizeof(int), hipMemcpyDeviceToDevice, s->st));
    HIPX(hipStreamSynchronize(s->st));
    return 0;
  }

  // Begin the context, walk `count` candidates from the chunk's first as t's link describes, drain the stream; the
  // thread's error text is kept in t.  keep_model: on the thread that has just walked c's own chunk (its device is set)
  void walk(bessx_session *c, ChunkRun &t, int count, bool keep_model = false) {
    t.rc = (keep_model || hipSetDevice(s->device) == hipSuccess) ? context_begin(c, keep_model) : fail(BESSX_ERR_HIP, "hipSetDevice");
    c->timing = s->timing;  // (its fills count in the session's score-pass statistics)
    if (t.rc == 0) t.rc = sequential_path(c, seq + t.lo, count, &lambda, 1, ic_type, 0, &t.res, &t.chain);
    if (t.rc == 0 && hipStreamSynchronize(c->st) != hipSuccess) t.rc = fail(BESSX_ERR_HIP, "chunk chain: stream");
    if (t.rc) t.err = g_err;
    t.last_len = t.chain.last_len;
    t.last_coef0 = t.chain.last_coef0;
  }

  int budget_of(int r) const { return std::max(8, (run[r].hi - run[r].lo) / 6); }

  // The stitch's first round, early (test hook kchunks_early_stitch=0 switches it off): the thread of chunk r - 1, when its
  // chunk is walked, re-fits the first candidates of chunk r from its own last model on its own (now idle) context while
  // the later chunks are still running -- what round 1 of the stitch below would do after ALL chunks have ended.  It
  // compares with the rows chunk r has stored by then (kchains_progress); a refit that could not see `budget` rows is
  // thrown away and done again in round 1.
  void early_stitch(int r) {  // on the thread and the context of chunk r - 1, which has just ended without error
    bessx_session *c = k->ctx[(size_t)r - 1];
    ChunkRun &q = run[(size_t)r], &t = early_st[(size_t)r];
    const int want = std::min(q.hi - q.lo, budget_of(r));
    const auto t0 = Clock::now();
    sp_leave(c);  // (this wait is not for the device: the other chains' shared passes must not wait for this thread)
    while (k->progress[r].load(std::memory_order_acquire) < want && k->ended[r].load(std::memory_order_acquire) == 0) {
      kchains_safe_point(c);  // (a chain that waits for every other chain to stand still must not wait for this one)
      std::this_thread::sleep_for(std::chrono::microseconds(20));
      if (secs(t0, Clock::now()) > s->wait_deadline_s) return;
    }
    if (k->ended[r].load(std::memory_order_acquire) == 2) return;
    const int rows = k->progress[r].load(std::memory_order_acquire);
    if (rows < want) return;
    t.shape(q.lo, q.hi, width);
    t.link_behind(run[(size_t)r - 1], &q, rows);  // (the rows chunk r has stored so far: final, it only appends)
    kchains_log(c, "early stitch of the next chunk", q.lo, rows);
    sp_join(c);
    walk(c, t, want, true);  // (its last fit's model IS the model the refit starts from)
    // a failure here is not the path's: round 1 of the stitch does this refit again
    if (t.rc == 0) early_ok[(size_t)r] = 1;
    else (void)hipGetLastError();
    kchains_log(c, "early stitch done", t.res.n_candidates, t.chain.stopped_at);
  }

  void chunk_job(int r) {
    if (r >= C) return;
    bessx_session *c = k->ctx[r];
    ChunkRun &q = run[r];
    const StartModel &m = start[(size_t)r];
    q.link(m.b.idx.data(), m.b.val.data(), (int)m.b.idx.size(), m.c0);
    kchains_log(c, "chunk starts", q.lo, q.hi);
    walk(c, q, q.hi - q.lo);
    kchains_log(c, "chunk ends", q.lo, q.hi);
    if (r < 10) k->ended[r].store(q.rc ? 2 : 1, std::memory_order_release);
    if (early_on && q.rc == 0 && r + 1 < C) early_stitch(r + 1);
    sp_leave(c);
    kchains_leave(k, q.rc != 0);
  }

  // ---- 2. the chunks side by side, on a stream and a host thread each.  Opens the shared-pass round: `scope`
  int chunk_round(std::optional<SharedPassScope> &scope) {
    if (int rc = writer_map_in_step()) return rc;
    if (lm_cov)
      for (bessx_session *c : k->ctx) c->cov[0].slot_w = staged ? s->kch_slot_w : nullptr;
    for (int r = 0; r < C; r++) run[r].shape(bounds[r], bounds[r + 1], width);
    kchains_round(k, C, staged);
    scope.emplace(s, k, C, lm_cov);
    early_on = C <= 9;
    if (const char *ee = test_hook("kchunks_early_stitch")) early_on = early_on && std::atoi(ee) != 0;
    early_st = std::vector<ChunkRun>((size_t)C);
    early_ok.assign((size_t)C, 0);
    for (int r = 0; r < 10; r++) {
      k->progress[r].store(0, std::memory_order_relaxed);
      k->ended[r].store(0, std::memory_order_relaxed);
    }
    if (!k->pool.run([this](int r) { chunk_job(r); }, s->wait_deadline_s))
      return fail(BESSX_ERR_HIP, "chunk chains: a host thread did not come back");
    for (int r = 0; r < C; r++)
      if (run[r].rc) return fail(run[r].rc, "chunk chain: " + run[r].err);
    t_chunks = Clock::now();
    return 0;
  }

  void stitch_job(int r, ChunkRun &t) {  // chunk r again, from its predecessor's last model as it stands before this round
    bessx_session *c = k->ctx[r];
    const ChunkRun &q = run[r];
    t.shape(q.lo, q.hi, width);
    t.link_behind(run[r - 1], &q, q.hi - q.lo);
    walk(c, t, std::min(q.hi - q.lo, budget_of(r)));
    sp_leave(c);
    kchains_leave(k, t.rc != 0);
  }

  // ---- 3. the stitch, in rounds until no chunk's last model changed (bess_amd.dist.StitchedKPath.step)
  // A chunk whose refit has not met its own chain after `budget` candidates is on another trajectory than the warm
  // chain (designs with many near-equivalent supports: correlated columns, weak signal) -- re-walking it, and then its
  // successors round by round, would cost more than the one chain.  The stitch then gives up: everything from the first
  // unsettled chunk on is walked as ONE chain from its predecessor's last model, and the session's automatic choice
  // becomes one chain.  (What a round decides: bessx_kplan.h, stitch_round.)
  int stitch_rounds() {
    std::vector<char> need((size_t)C, 1);
    need[0] = 0;
    for (int round = 1;; round++) {
      std::vector<ChunkRun> st((size_t)C);
      std::vector<char> todo((size_t)C, 0);  // the refits of this round that are not there already (the early stitch)
      std::vector<bessx_session *> who;
      for (int r = 1; r < C; r++) {
        if (round == 1 && early_ok[(size_t)r]) {
          st[(size_t)r] = std::move(early_st[(size_t)r]);
        } else if (need[r]) {
          todo[(size_t)r] = 1;
          who.push_back(k->ctx[r]);
        }
      }
      if (!who.empty()) {
        if (int rc = writer_map_in_step()) return rc;
        kchains_round(k, (int)who.size(), staged);
        sp_round(k, who);
        auto job = [&](int r) {
          if (r < C && todo[(size_t)r]) stitch_job(r, st[(size_t)r]);
        };
        if (!k->pool.run(job, s->wait_deadline_s)) return fail(BESSX_ERR_HIP, "chunk chains: a host thread did not come back");
      }
      std::vector<StitchRefit> refit((size_t)C);
      for (int r = 1; r < C; r++) {
        if (!need[r]) continue;
        ChunkRun &q = run[r], &t = st[r];
        if (t.rc) return fail(t.rc, "chunk chain (stitch): " + t.err);
        const int m = std::min(t.res.n_candidates, q.hi - q.lo);
        std::copy_n(t.T0.begin(), m, q.T0.begin());  // what was walked before the merge point is replaced
        std::copy_n(t.iters.begin(), m, q.iters.begin());
        std::copy_n(t.lam.begin(), m, q.lam.begin());
        std::copy_n(t.loss.begin(), m, q.loss.begin());
        std::copy_n(t.ic.begin(), m, q.ic.begin());
        std::copy_n(t.coef0.begin(), m, q.coef0.begin());
        std::copy_n(t.support.begin(), (size_t)m * width, q.support.begin());
        std::copy_n(t.beta.begin(), (size_t)m * width, q.beta.begin());
        refits += m;
        refit[(size_t)r] = {m, q.hi - q.lo, t.chain.stopped_at >= 0};
      }
      const StitchRound d = stitch_round(need, refit);
      for (int r = 1; r < C; r++)
        if (d.changed[r]) {  // its last model is a new one
          run[r].last_idx = st[r].last_idx;
          run[r].last_val = st[r].last_val;
          run[r].last_len = st[r].last_len;
          run[r].last_coef0 = st[r].last_coef0;
        }
      give_up_from = d.give_up_from;
      if (give_up_from >= 0 || !d.any) return 0;
      if (round > C) return fail(BESSX_ERR_NUMERIC, "chunk chains: the stitching did not settle");
      need = d.need;
    }
  }

  // after a give-up: the rest as ONE chain on the session's own state, from the last settled chunk's last model, on the
  // warm cache
  int give_up_tail() {
    if (give_up_from < 1) return 0;
    const int f = give_up_from;
    ChunkRun tail;
    tail.shape(bounds[f], ns, width);
    tail.link_behind(run[f - 1]);
    kchains_quiesce(s);
    if (int rc = settle_device_chain(s)) return rc;
    for (auto &q : s->cache) q.valid = q.model_only = false;
    s->dev_state_rs = -1;
    if (int rc = sequential_path(s, seq + bounds[f], ns - bounds[f], &lambda, 1, ic_type, 0, &tail.res, &tail.chain)) return rc;
    tail.last_len = tail.chain.last_len;
    tail.last_coef0 = tail.chain.last_coef0;
    run.resize((size_t)f);
    run.push_back(std::move(tail));
    s->kch_giveups++;
    if (s->kpath_chains == 0) s->kch_auto_off = true;
    return 0;
  }

  // ---- the path's result: the candidates in order, the best of them by the criterion (first minimum, :113)
  void assemble(bessx_path_result *res) {
    if (k->log_on) {
      kchains_log(s, "path ends", 0, 0);
      for (const auto &r : k->log) std::fprintf(stderr, "kchunks %8.3f ms  chain %2d  %-28s %d %d\n", r.ms, r.chain, r.what, r.a, r.b);
    }
    s->kch_t[0] += secs(t_begin, t_coarse);
    s->kch_t[1] += secs(t_coarse, t_chunks);
    s->kch_t[2] += secs(t_chunks, Clock::now());
    res->n_candidates = 0;
    int best_r = 0, best_i = 0;
    for (size_t r = 0; r < run.size(); r++) {  // (fewer chunks than C after a give-up)
      const ChunkRun &q = run[r];
      for (int i = 0; i < q.hi - q.lo; i++) {
        const int g = res->n_candidates++;
        iters_path += std::min(q.iters[i], s->max_iter);  // (a fit that ran out of iterations reports max_iter + 1)
        if (q.ic[i] < run[best_r].ic[best_i]) {
          best_r = (int)r;
          best_i = i;
        }
        if (g >= res->capacity) continue;
        if (res->cand_T0) res->cand_T0[g] = q.T0[i];
        if (res->cand_lambda) res->cand_lambda[g] = q.lam[i];
        if (res->cand_iters) res->cand_iters[g] = q.iters[i];
        if (res->cand_train_loss) res->cand_train_loss[g] = q.loss[i];
        if (res->cand_ic) res->cand_ic[g] = q.ic[i];
        if (res->cand_coef0) res->cand_coef0[g] = q.coef0[i];
        for (int j = 0; j < res->max_T0; j++) {
          if (res->cand_support) res->cand_support[(size_t)g * res->max_T0 + j] = j < width ? q.support[(size_t)i * width + j] : -1;
          if (res->cand_beta) res->cand_beta[(size_t)g * res->max_T0 + j] = j < width ? q.beta[(size_t)i * width + j] : 0.0;
        }
      }
    }
    const ChunkRun &q = run[best_r];
    if (res->beta) {
      std::fill(res->beta, res->beta + s->p_full, 0.0);
      for (int j = 0; j < width; j++) {
        const int col = q.support[(size_t)best_i * width + j];
        if (col >= 0) res->beta[col] = q.beta[(size_t)best_i * width + j];
      }
    }
    res->coef0 = q.coef0[best_i];
    res->train_loss = q.loss[best_i];
    res->ic = q.ic[best_i];
    res->lambda = q.lam[best_i];
    res->best_T0 = q.T0[best_i];
    res->best_iters = q.iters[best_i];
  }

  // the session as the path leaves it.  Fits and get_A calls as the single chain counts them; the work really done
  // (coarse chain, replaced candidates) is in bessx_session_counter 14-16
  void session_state(bessx_path_chain *link) {
    s->n_fits = ns;
    s->n_iters = iters_path;
    s->kch_paths++;
    s->kch_last_chains = C;
    s->kch_refits += refits;
    // the session's own device state is the coarse chain's last fit, not the path's last candidate
    for (auto &q : s->cache) q.valid = q.model_only = false;
    s->dev_state_rs = -1;
    const ChunkRun &q = run.back();
    if (link) {  // the model the link's successor starts from
      link->last_len = q.last_len;
      link->last_coef0 = q.last_coef0;
      for (int i = 0; i < q.last_len && i < link->last_cap; i++) {
        if (link->last_idx) link->last_idx[i] = q.last_idx[i];
        if (link->last_val) link->last_val[i] = q.last_val[i];
      }
    }
    // Algorithm state as the path leaves it: the last candidate's model (normalised scale)
    s->beta.idx.assign(q.last_idx.begin(), q.last_idx.begin() + q.last_len);
    s->beta.val.assign(q.last_val.begin(), q.last_val.begin() + q.last_len);
    s->coef0 = q.last_coef0;
  }
};

// statistics of a chain context belong to the session
void fold_context_statistics(bessx_session *s, bessx_session *c) {
  auto take = [](auto &to, auto &from) { to += from, from = 0; };
  take(s->cov_panel_groups, c->cov_panel_groups);
  take(s->cov_cg_fallbacks, c->cov_cg_fallbacks);
  take(s->cov_tie_rescues, c->cov_tie_rescues);
  take(s->dbg_waits, c->dbg_waits);
  take(s->dbg_waits_ready, c->dbg_waits_ready);
  take(s->dbg_enq_s, c->dbg_enq_s);
  take(s->chain_queued, c->chain_queued);
  take(s->chain_hits, c->chain_hits);
  take(s->n_submodel_steps, c->n_submodel_steps);
  take(s->k1_seconds, c->k1_seconds);
  take(s->k1_bytes, c->k1_bytes);
  take(s->k1_launches, c->k1_launches);
  for (int w = 0; w < 2; w++) {
    take(s->panel_w_seconds[w], c->panel_w_seconds[w]);
    take(s->panel_w_launches[w], c->panel_w_launches[w]);
  }
}

}  // namespace

int sequential_path_chunked(bessx_session *s, const int *seq, int ns, double lambda, int ic_type,
                            bessx_path_result *res, bessx_path_chain *link) {
  const int C = chains_for(s, ns, link != nullptr, link && link->init_len > 0 && link->keep_caches);
  HIPX(hipSetDevice(s->device));
  KChains *k = s->kch;
  if (!k || (int)k->ctx.size() < C || k->pool.broken)
    return fail(BESSX_ERR_HIP, "chunk chains: not prepared (kchunks_prepare)");
  const int width = res->max_T0 > 0 ? res->max_T0 : seq[ns - 1];
  ChunkPath d{s, k, seq, ns, lambda, ic_type, C, width, s->model_type == 1 && s->cov_mode};
  d.plan();
  d.fill_stream();
  if (int rc = d.coarse_chain(link)) return rc;
  std::optional<SharedPassScope> scope;  // opened by chunk_round: from there EVERY way out closes the shared-pass round
  if (int rc = d.chunk_round(scope)) return rc;
  if (int rc = d.stitch_rounds()) return rc;
  if (int rc = d.give_up_tail()) return rc;
  if (int rc = scope->close()) return rc;
  d.assemble(res);
  for (bessx_session *c : k->ctx) fold_context_statistics(s, c);
  d.session_state(link);
  return 0;
}

}  // namespace bessx

