// The root solve: the host readback of residual norms, the two Broyden drivers over one shared skeleton, the Banach
// fallback, the fc block kernel's driver, and the C-ABI entries that solve.
//
// Reference mapping (implicit_block.py unless noted):
//   inf_root_find         <- RootFind.apply -> broyden_find_root -> broyden              (:51-100)
//   inf_imblock_forward   <- imBlock.forward value path                                  (:220-230)
//   inf_imblock_backward  <- imBlock.Backward.backward                                   (:176-217)
//   inf_banach_find_root  <- banach_find_root -> find_fixed_point                        (:17-28,57-65)
//   broyden_core          <- broyden(..., ls=False)                                      (broyden.py:123-193)
//   broyden_core_ls       <- broyden(..., ls=True): line_search, scalar_search_armijo    (broyden.py:24-99)
//   inf_broyden_update    <- the rank-1 update and matvec                                (broyden.py:174-181)
//   inf_broyden_line_step <- x_est = x0 + s * update                                     (broyden.py:70-72)
#include <chrono>
#include <thread>

#include "engine.h"

using namespace inf;

namespace {

// per-sample sums of squares (partials in bf.part) -> host (the reference's .item() per iteration).
// Asynchronous form: the reduction and a D2H copy into pinned host memory are enqueued and an event marks
// them; wait_sumsq blocks on that event.  Two slots per host thread let the Broyden loop keep one
// speculative iteration in flight (broyden_core).  Slots are per thread, so concurrent callers on different
// threads never share one.
struct SumsSlot {
  double* host = nullptr;
  hipEvent_t ev = nullptr;
  int cap = 0;
};
thread_local SumsSlot g_sums_slots[2];
int sums_slot(int i, int B, SumsSlot** out) {
  SumsSlot& sl = g_sums_slots[i & 1];
  if (sl.cap < B + 1) {
    if (sl.host) (void)hipHostFree(sl.host);
    sl.host = nullptr;
    const int cap = std::max(B + 1, 1024);
    // coherent: the fc residual launches write their per-sample sums straight into it (broyden_core, zero-copy)
    if (hipHostMalloc(reinterpret_cast<void**>(&sl.host), sizeof(double) * cap, hipHostMallocCoherent) != hipSuccess)
      return INF_ERR_HIP;
    sl.cap = cap;
  }
  if (!sl.ev && hipEventCreateWithFlags(&sl.ev, INF_EV_SYNC) != hipSuccess) return INF_ERR_HIP;
  *out = &sl;
  return INF_OK;
}
// The per-sample stopping decision of step k (INF_CONV_PER_SAMPLE), queued between the reduction and the
// readback: the device state machine (broyden.hip ps_decide_kernel) and the copy of the improved samples'
// iterate (and f) into the lowest-iterate buffers.  The readback then carries the count of samples iterating.
struct PsStep {
  bool on = false;
  int k = 0, T = 0;
  double eps = 0.0;          // eps * sqrt(d)
  const float* x = nullptr;  // the iterate of this residual
  const float* f = nullptr;  // its f (nullable)
  long sb = 0, si = 0;
};
int enqueue_sumsq(InfNet* f, int B, Bufs& bf, SumsSlot* sl, hipStream_t s, const PsStep* ps = nullptr) {
  // narrow fc nets write one partial per sample: with the global rule those are the sums already (0 + x == x for the
  // non-negative or NaN sums), so the readback takes them directly and the reduction launch is skipped (wide fc nets
  // write chunk partials, as conv nets)
  const bool ps_on = ps && ps->on;
  const bool direct = ((f->fc && bf.nchunk == 1) || bf.sample_sums) && !ps_on;
  if (direct && bf.part == sl->host) {               // the residual launch wrote the sums into the slot itself
    const bool bound = bf.stop_bound && bf.stop_ev == sl->ev;
    bf.stop_bound = false;
    if (bound) return INF_OK;                        // ... and its launch completes the event (no marker packet: the
                                                     // marker after a launch idles the GPU ~4.4 us)
    INF_HIP(hipEventRecord(sl->ev, s));
    return INF_OK;
  }
  if (!direct && !ps_on) {                            // global rule: the reduction writes the sums into the slot
    bool bound = false;                              // (and completes the slot's event itself: no marker packet)
    INF_TRY(launch_reduce_partials(bf.part, B, bf.nchunk, sl->host, s, sl->ev, &bound));
    if (!bound) INF_HIP(hipEventRecord(sl->ev, s));
    return INF_OK;
  }
  if (!direct) INF_TRY(launch_reduce_partials(bf.part, B, bf.nchunk, bf.sumsq, s));
  int n = B;
  if (ps_on) {
    INF_TRY(launch_ps_decide(bf.sumsq, bf.ps_state, bf.ps_active, bf.ps_improved, B, ps->k, ps->T, ps->eps, s));
    INF_TRY(launch_ps_copy(bf.ps_improved, ps->x, ps->f, bf.ps_lowx, bf.ps_lowf, B, f->d, ps->sb, ps->si, s));
    n = B + 1;
  }
  INF_HIP(hipMemcpyAsync(sl->host, direct ? bf.part : bf.sumsq, sizeof(double) * n, hipMemcpyDeviceToHost, s));
  INF_HIP(hipEventRecord(sl->ev, s));
  return INF_OK;
}
// n_active (may be null): the per-sample mode's count of samples still iterating after this step
int wait_sumsq(SumsSlot* sl, int B, std::vector<double>& host_sumsq, int* n_active = nullptr) {
  INF_TRY(host_wait(sl->ev));
  memcpy(host_sumsq.data(), sl->host, sizeof(double) * B);
  if (n_active) *n_active = (int)sl->host[B];
  return INF_OK;
}
int read_sumsq(InfNet* f, int B, Bufs& bf, std::vector<double>& host_sumsq, hipStream_t s) {
  SumsSlot* sl = nullptr;
  INF_TRY(sums_slot(0, B, &sl));
  INF_TRY(enqueue_sumsq(f, B, bf, sl, s));
  return wait_sumsq(sl, B, host_sumsq);
}

// residual evaluation g = x_embed - f(z) - z (+ dg = g - g_prev), f(z) kept in bf.fcur, per-sample partial sums of
// squares in bf.part.  zsub is the subtracted "- z" term: z itself for Broyden, zeros for the Banach map.
OutArgs resid_out(const float* zsub, const float* xemb, float* gout, float* dg, const float* gprev, Bufs& bf) {
  OutArgs a;
  memset(&a, 0, sizeof(a));
  a.in0 = xemb;
  a.in1 = zsub;
  a.in2 = gprev;
  a.out0 = gout;
  a.out1 = dg;
  a.out2 = bf.fcur;
  a.partial = bf.part;
  a.nchunk = bf.nchunk;
  a.sample_sums = bf.sample_sums;
  a.stop_ev = bf.stop_ev;
  a.stop_bound = &bf.stop_bound;
  return a;
}
int eval_resid_part(InfNet* f, const float* z, const float* zsub, const float* xemb, float* gout, float* dg,
                    const float* gprev, int B, Bufs& bf, hipStream_t s) {
  const OutArgs a = resid_out(zsub, xemb, gout, dg, gprev, bf);
  return run_forward(f, z, B, bf, OM_RESID, &a, s);
}
// the same, synchronously, with the per-sample sums of squares on the host
int eval_resid(InfNet* f, const float* z, const float* zsub, const float* xemb, float* gout, float* dg,
               const float* gprev, int B, Bufs& bf, std::vector<double>& host_sumsq, hipStream_t s) {
  INF_TRY(eval_resid_part(f, z, zsub, xemb, gout, dg, gprev, B, bf, s));
  return read_sumsq(f, B, bf, host_sumsq, s);
}

// vjp residual of the implicit backward (implicit_block.py:186-190): g = (y + y^T J) - grad
int vjp_resid_part(InfNet* f, const float* y, const float* zi, const float* gradi, float* gout, float* dg,
                   const float* gprev, int B, Bufs& bf, hipStream_t s) {
  INF_TRY(run_vjp(f, y, bf.tmp, zi, nullptr, nullptr, B, bf, s));
  return launch_vjp_resid(bf.tmp, y, gradi, gprev, gout, dg, bf.part, B, f->d, bf.nchunk, f->fc, s);
}

double total(const std::vector<double>& v) {
  double t = 0.0;
  for (double x : v) t += x;
  return t;
}

// Broyden root find on internal-layout buffers.  Solves z with g(z) = xemb - f(z) - z = 0.
// Result (lowest iterate) in bf.lowest.  y (internal) is the Banach fallback start.
// resid(x, gout, dg, gprev): residual g(x) -> gout (+ dg = g - gprev when gprev), per-sample partial sums of
// squares -> bf.part, and (root solves) f(x) -> bf.fcur.  broyden_core reduces and reads them back.
using ResidFn = std::function<int(const float* x, float* gout, float* dg, const float* gprev)>;
// update + residual in one launch (fused fc nets): the update ba computes ba.xnew, then the residual at it, as resid
using StepFn = std::function<int(const BroydenArgs& ba, float* gout, float* dg, const float* gprev)>;
// Broyden's start in one launch: x0 = 0, g0 = g(x0) (+ f(x0) in bf.fcur, partials in bf.part), update = -g0,
// x1 = x0 + update, dx = x1 - x0
using StartFn = std::function<int(float* x0, float* g0, float* upd, float* x1, float* dx)>;

// Copies the per-sample results (INF_CONV_PER_SAMPLE) into the stats and the caller's optional host arrays.
int ps_collect(Bufs& bf, int B, int T, InfBroydenStats& stats, std::vector<double>& lowest_ss, hipStream_t s) {
  const int stride = PS_HEAD + T;
  std::vector<double> st((size_t)B * stride);
  INF_HIP(hipMemcpyAsync(st.data(), bf.ps_state, sizeof(double) * st.size(), hipMemcpyDeviceToHost, s));
  INF_HIP(hipStreamSynchronize(s));
  int nmax = 0, lmax = 0, prot = 0;
  double d2 = 0.0;
  lowest_ss.assign(B, 0.0);
  for (int b = 0; b < B; ++b) {
    const double* p = st.data() + (size_t)b * stride;
    const int ns = (int)p[3], ls = (int)p[4], pb = (int)p[5];
    nmax = std::max(nmax, ns);
    lmax = std::max(lmax, ls);
    prot |= pb;
    lowest_ss[b] = p[1] * p[1];
    d2 += lowest_ss[b];
    if (stats.sample_nstep) stats.sample_nstep[b] = ns;
    if (stats.sample_lowest_step) stats.sample_lowest_step[b] = ls;
    if (stats.sample_prot_break) stats.sample_prot_break[b] = pb;
  }
  stats.nstep = nmax;
  stats.tnstep = nmax;
  stats.lowest_step = lmax;
  stats.prot_break = prot;
  stats.diff = sqrt(d2);
  return INF_OK;
}

// zeroes the stats, keeping the caller's per-sample arrays
void reset_stats(InfBroydenStats& stats) {
  int *a = stats.sample_nstep, *b = stats.sample_lowest_step, *c = stats.sample_prot_break;
  memset(&stats, 0, sizeof(stats));
  stats.sample_nstep = a;
  stats.sample_lowest_step = b;
  stats.sample_prot_break = c;
}

// The stop decision of broyden.py:159-172 after an iteration whose objective is trace.back() == obj
enum class Stop { GO, CONVERGED, STALLED, PROT_BREAK };
Stop broyden_stop(double obj, double eps, double init, int nstep, int T, const std::vector<double>& trace) {
  if (obj < eps) return Stop::CONVERGED;                              // :163-164
  if (obj < 3 * eps && nstep == T) {                                  // :165-168
    const size_t k0 = trace.size() > (size_t)T ? trace.size() - T : 0;
    double mx = trace[k0], mn = trace[k0];
    for (size_t k = k0; k < trace.size(); ++k) {
      mx = std::max(mx, trace[k]);
      mn = std::min(mn, trace[k]);
    }
    if (mx / mn < 1.3) return Stop::STALLED;
  }
  if (obj > init * 1e6) return Stop::PROT_BREAK;                      // :169-172
  return Stop::GO;
}

// What the two Broyden drivers share (the global rule's bookkeeping of broyden.py:123-193).  Iterates rotate through
// {xa, xb, lowest} and f(z) through {fcur, flow, fspec}; the lowest iterate (:159-162) is tracked by pointer and the
// Bufs pointers are permuted at the end so that bf.lowest / bf.flow name the result.
struct BroydenRun {
  InfNet* f;
  const int B, T;
  const size_t E;
  Bufs& bf;
  InfBroydenStats& stats;
  std::vector<double>& lowest_ss;
  const double eps;                                                   // broyden.py:131
  float* xpool[3];
  float* fpool[3];
  float* low = nullptr;                                               // the lowest iterate
  float* flow = nullptr;                                              // its f (null: not kept)
  double init = 0.0, lowest = 0.0;
  int lowest_step = 0;
  std::vector<double> trace;

  BroydenRun(InfNet* f_, int B_, int T_, double eps_in, InfBroydenStats& st, std::vector<double>& lss, Bufs& bf_)
      : f(f_), B(B_), T(T_), E((size_t)B_ * f_->d), bf(bf_), stats(st), lowest_ss(lss),
        eps(eps_in * sqrt((double)((size_t)B_ * f_->d))), xpool{bf_.xa, bf_.xb, bf_.lowest},
        fpool{bf_.fcur, bf_.flow, bf_.fspec} {
    reset_stats(stats);
  }
  // a pool buffer that is neither a nor b
  static float* pick(float* const* pool, const float* a, const float* b) {
    for (int i = 0; i < 3; ++i)
      if (pool[i] != a && pool[i] != b) return pool[i];
    return pool[0];
  }
  // low-rank update from iterate `step` (x = xfrom, g = gfrom) to xto (broyden.py:174-181)
  BroydenArgs update_args(int step, float* xfrom, float* gfrom, float* xto, const int* active = nullptr) const {
    BroydenArgs ba;
    memset(&ba, 0, sizeof(ba));
    ba.batch = B;
    ba.d = f->d;
    ba.T = T;
    ba.sb = f->fc ? 1 : f->d;
    ba.si = f->fc ? B : 1;
    ba.cs = (long)E;
    ba.U = bf.U;
    ba.VT = bf.VT;
    ba.dx = bf.dx;
    ba.dg = bf.dg;
    ba.gx = gfrom;
    ba.x = xfrom;
    ba.xnew = xto;
    ba.dxnew = bf.dx;
    ba.upd = bf.upd;
    ba.part = bf.bpart;
    ba.m = (step - 1) % T;
    ba.ncols = std::min(step, T);
    ba.active = active;
    return ba;
  }
  // the initial residual's sums: returns the initial objective
  double begin(const std::vector<double>& ss) {
    init = lowest = sqrt(total(ss));
    lowest_ss = ss;
    trace.assign(1, init);
    return init;
  }
  // records iterate x (its f in fx, null when f is not kept) of step nstep if it is the lowest (:159-162)
  void record(double obj, int nstep, float* x, float* fx, const std::vector<double>& ss) {
    if (!(obj < lowest)) return;
    low = x;
    if (fx) flow = fx;
    lowest = obj;
    lowest_step = nstep;
    lowest_ss = ss;
  }
  Stop stop(double obj, int nstep) {
    const Stop st = broyden_stop(obj, eps, init, nstep, T, trace);
    if (st == Stop::PROT_BREAK) stats.prot_break = 1;
    return st;
  }
  void write_trace() {
    stats.n_trace = (int)std::min<size_t>(trace.size(), 64);
    for (int k = 0; k < stats.n_trace; ++k) stats.trace[k] = trace[k];
  }
  // names the result: bf.lowest = the lowest iterate, bf.flow = its f; the other buffers become scratch
  void finish(int nstep, int tnstep) {
    float* rest[2];
    int k = 0;
    for (float* p : xpool)
      if (p != low && k < 2) rest[k++] = p;
    bf.lowest = low;
    bf.xa = rest[0];
    bf.xb = rest[1];
    float* fr[2];
    k = 0;
    float* fl = flow ? flow : fpool[1];
    for (float* p : fpool)
      if (p != fl && k < 2) fr[k++] = p;
    bf.flow = fl;
    bf.fcur = fr[0];
    bf.fspec = fr[1];
    stats.nstep = nstep;
    stats.tnstep = tnstep;
    stats.lowest_step = lowest_step;
    stats.diff = lowest;
  }
};

// broyden.py:123-193 with the residual as a callback; the result (lowest iterate) is in bf.lowest.
// f->convergence selects the stopping rule: INF_CONV_GLOBAL is the reference's (one Frobenius norm over the
// batch against eps sqrt(B d), one lowest iterate for the batch); INF_CONV_PER_SAMPLE runs the same rules per
// sample against eps sqrt(d) (the reference's result for a batch of one, i.e. independent of how the batch is
// sharded), with the decisions taken on the device (ps_decide_kernel) and stopped samples frozen.
// stats.sample_* (host arrays, nullable) receive the per-sample outcome in that mode.
int broyden_core(InfNet* f, const ResidFn& resid, int B, int T, double eps_in, InfBroydenStats& stats,
                 std::vector<double>& lowest_ss, Bufs& bf, hipStream_t s, bool keep_f = false,
                 const StepFn* step_fn = nullptr, const StartFn* start_fn = nullptr, SpecTail* tail = nullptr,
                 bool resid_sample_sums = false) {
  const bool per_sample = f->convergence == INF_CONV_PER_SAMPLE;
  std::vector<double> ss(B);
  lowest_ss.assign(B, 0.0);
  BroydenRun br(f, B, T, eps_in, stats, lowest_ss, bf);
  const size_t E = br.E;
  const double eps = br.eps;
  const double eps_ps = eps_in * sqrt((double)f->d);                 // the same rule for a batch of one
  stats.eps = per_sample ? eps_ps : eps;
  stats.convergence = f->convergence;

  // One iteration of lookahead: while the host waits for iteration k's residual norm (the reference's
  // .item(), broyden.py:157), iteration k+1's low-rank update and residual are already queued behind it, so
  // the GPU does not idle through the host round trip.  If k stops the loop, k+1's work is discarded: it
  // only wrote scratch (per-sample mode: the device decisions of step k already froze every sample it
  // stopped).  The decided lowest, the pending and the speculative iterate (and f) are always distinct pool
  // buffers (per-sample mode: the lowest is copied per sample into ps_lowx / ps_lowf).
  float* const* xpool = br.xpool;
  float* const* fpool = br.fpool;
  const auto pick = BroydenRun::pick;
  SumsSlot* slot[2];
  INF_TRY(sums_slot(0, B, &slot[0]));
  INF_TRY(sums_slot(1, B, &slot[1]));
  PsStep ps;
  ps.on = per_sample;
  ps.T = T;
  ps.eps = eps_ps;
  ps.sb = f->fc ? 1 : f->d;
  ps.si = f->fc ? B : 1;
  auto sums = [&](int k, const float* xk, const float* fk, SumsSlot* sl) {
    ps.k = k;
    ps.x = xk;
    ps.f = keep_f ? fk : nullptr;
    return enqueue_sumsq(f, B, bf, sl, s, &ps);
  };
  float *gx = bf.ga, *gn = bf.gb;
  float* x = xpool[0];
  br.low = per_sample ? bf.ps_lowx : x;
  // (U / VT need no zeroing: every update reads only the columns j < m, j < ncols that earlier steps of this solve
  // wrote, as broyden.py:174-181 reads Us[..., :nstep - 1])
  // the one-launch start (fc nets, global rule: nothing is queued between the residual and the first step)
  const bool fused_start = start_fn && !per_sample && T > 0;
  if (!fused_start) INF_HIP(hipMemsetAsync(x, 0, sizeof(float) * E, s));
  bf.fcur = fpool[0];
  // zero-copy readback (fc nets, global rule): each residual launch writes its per-sample sums straight into the
  // pinned slot its norm is read from (bf.part points there while it is enqueued), so no copy launch sits between
  // the residual and the event the host waits on; bf.part is restored on every return path
  // conv nets whose residual launches can write per-sample totals (resid_sample_sums: the root solve's
  // eval_resid_part / resid_bcast, d <= 4 residual chunks per sample): the residual launch itself sums each sample
  // over its chunks (one block per sample, conv_out_resid_sample_kernel) into the slot, so no reduction launch sits
  // between it and the readback either.  (The implicit backward's residual writes chunk partials: not here.)
  const bool zc = ((f->fc && bf.nchunk == 1) || (!f->fc && resid_sample_sums && out_nchunk(f->d) <= 4)) && !per_sample;
  struct PartRestore {
    Bufs& b;
    double* p;
    hipEvent_t e;
    ~PartRestore() {
      b.part = p;
      b.stop_ev = e;
      b.stop_bound = false;
      b.sample_sums = false;
    }
  } part_restore{bf, bf.part, bf.stop_ev};
  auto target = [&](SumsSlot* sl) {
    if (zc) {
      bf.part = sl->host;
      bf.stop_ev = sl->ev;
      bf.sample_sums = !f->fc;
    }
  };
  target(slot[0]);
  float *xp = nullptr, *fp = nullptr;
  if (fused_start) {
    xp = pick(xpool, br.low, x);
    INF_TRY((*start_fn)(x, gx, bf.upd, xp, bf.dx));
  } else {
    INF_TRY(resid(x, gx, nullptr, nullptr));
  }
  INF_TRY(sums(0, x, bf.fcur, slot[0]));
  if (keep_f) br.flow = per_sample ? bf.ps_lowf : bf.fcur;
  // iteration 1 is queued before the initial norm is read (update = -g0, x1 = x0 + update, :144)
  if (T > 0) {
    if (!fused_start) {
      xp = pick(xpool, br.low, x);
      INF_TRY(launch_neg(gx, bf.upd, (long)E, s));
      INF_TRY(launch_axpy_step(x, bf.upd, xp, bf.dx, (long)E, s));
    }
    fp = pick(fpool, br.flow, bf.fcur);
    bf.fcur = fp;
    target(slot[1]);
    INF_TRY(resid(xp, gn, bf.dg, gx));
    INF_TRY(sums(1, xp, fp, slot[1]));
  }
  int n_active = B;
  INF_TRY(wait_sumsq(slot[0], B, ss, per_sample ? &n_active : nullptr));
  double obj = br.begin(ss);
  int nstep = 0;
  const int* active = per_sample ? bf.ps_active : nullptr;
  const bool go = per_sample ? (n_active > 0 && T > 0) : (obj >= eps && nstep < T);   // broyden.py:153
  if (go) {
    int ps_ = 1;
    double prev_obj = -1.0;
    for (;;) {
      // pending = iteration nstep + 1 (iterate xp, residual in gn, f in fp, norms in slot[ps_]).  The next
      // iteration is queued before the pending norm is read, unless the threshold forbids it or the
      // observed contraction predicts that the pending iteration converges (then it would be wasted work).
      const bool allow = nstep + 1 < T;
      const bool likely_last = !per_sample && prev_obj > 0.0 && obj * (obj / prev_obj) < eps;
      float *xs = nullptr, *fs = nullptr;
      auto enqueue_next = [&](int pending_step) -> int {
        target(slot[1 - ps_]);
        xs = pick(xpool, br.low, xp);
        fs = pick(fpool, br.flow, fp);
        if (step_fn) {
          bf.fcur = fs;
          INF_TRY((*step_fn)(br.update_args(pending_step, xp, gn, xs, active), gx, bf.dg, gn));
        } else {
          INF_TRY(launch_broyden_update(br.update_args(pending_step, xp, gn, xs, active), s));
          bf.fcur = fs;
          INF_TRY(resid(xs, gx, bf.dg, gn));
        }
        return sums(pending_step + 1, xs, fs, slot[1 - ps_]);
      };
      const bool spec = allow && !likely_last;
      if (spec) {
        INF_TRY(enqueue_next(nstep + 1));
      } else if (tail && tail->fn && !per_sample && keep_f) {
        INF_TRY(tail->fn(xp, fp));
        tail->x = xp;
        tail->f = fp;
      }
      INF_TRY(wait_sumsq(slot[ps_], B, ss, per_sample ? &n_active : nullptr));
      nstep += 1;
      x = xp;
      prev_obj = obj;
      obj = sqrt(total(ss));
      br.trace.push_back(obj);
      if (per_sample) {
        if (n_active == 0 || !allow) break;
      } else {
        br.record(obj, nstep, xp, keep_f ? fp : nullptr, ss);
        if (br.stop(obj, nstep) != Stop::GO || !allow) break;          // (!allow: nstep == T)
      }
      if (!spec) {
        // the loop goes on past the iterate the tail was queued for: that iterate is no longer the candidate result,
        // and its buffers go back to the pools (a later iterate may reuse them), so the tail no longer names it
        if (tail) tail->x = tail->f = nullptr;
        INF_TRY(enqueue_next(nstep));
      }
      xp = xs;
      fp = fs;
      ps_ = 1 - ps_;
      std::swap(gx, gn);                                                // gn: the new pending residual
    }
  }
  br.write_trace();
  if (per_sample) {
    // the pool buffers are scratch; the result is the per-sample lowest iterate
    bf.lowest = bf.ps_lowx;
    bf.flow = bf.ps_lowf;
    bf.xa = xpool[0];
    bf.xb = xpool[1];
    bf.fcur = fpool[0];
    bf.fspec = fpool[2];
    return ps_collect(bf, B, T, stats, lowest_ss, s);
  }
  br.finish(nstep, nstep);
  return INF_OK;
}

// _safe_norm(g)**2 (broyden.py:18-21,81) from the per-sample sums of squares: the fp32 norm squared in fp32, inf when
// any entry is not finite
float ls_phi(const std::vector<double>& ss) {
  const double t = total(ss);
  if (!std::isfinite(t)) return INFINITY;
  const float n = (float)sqrt(t);
  return n * n;
}

// broyden.py:123-193 with line_search(on=True) (:66-99) and scalar_search_armijo (:24-63; c1 = 1e-4, alpha0 = 1,
// amin = 1e-2, derphi0 = -phi0), the global rule.  Each step: the trial point x0 + s update (launch_line_step; s = 1 is
// the update launch's own x + update), its residual and norm read back (one host round trip per evaluation: the step
// size decides the next point, so nothing is speculated), the quadratic then cubic backtracking in fp32 as the
// reference's 0-d fp32 tensors compute it, the last evaluation reused when the accepted step is the stored one (:77-78,
// 95-96).  A failed search takes the full step with ite = 0 and evaluates it again (:90-98).  stats.tnstep counts
// nstep + the accepted searches' extra iterations (:156).  Result (lowest iterate) in bf.lowest, its f in bf.flow.
// (Compiled uncontracted: the build's -ffp-contract=fast would fuse the search's fp32 products and sums, which the
// reference rounds one by one.)
int broyden_core_ls(InfNet* f, const ResidFn& resid, int B, int T, double eps_in, InfBroydenStats& stats,
                    std::vector<double>& lowest_ss, Bufs& bf, hipStream_t s, bool keep_f) {
#pragma clang fp contract(off)
  BroydenRun br(f, B, T, eps_in, stats, lowest_ss, bf);
  const size_t E = br.E;
  const double eps = br.eps;
  stats.eps = eps;
  stats.convergence = INF_CONV_GLOBAL;
  float* const* xpool = br.xpool;
  float* const* fpool = br.fpool;
  const auto pick = BroydenRun::pick;
  float* x = xpool[0];
  float* fx = fpool[0];
  float *gx = bf.ga, *gt = bf.gb;
  std::vector<double> ss(B), ss_t(B);
  INF_HIP(hipMemsetAsync(x, 0, sizeof(float) * E, s));
  bf.fcur = fx;
  INF_TRY(resid(x, gx, nullptr, nullptr));
  INF_TRY(read_sumsq(f, B, bf, ss, s));
  double obj = br.begin(ss);
  br.low = x;
  br.flow = keep_f ? fx : nullptr;
  int nstep = 0, tnstep = 0;
  INF_TRY(launch_neg(gx, bf.upd, (long)E, s));                      // update = -gx (:144)
  float* xt = pick(xpool, br.low, x);
  INF_TRY(launch_axpy_step(x, bf.upd, xt, bf.dx, (long)E, s));       // the s = 1 trial point
  bool xt_full = true;                                               // xt holds x + 1 * update
  while (obj >= eps && nstep < T) {                                  // :153
    // ---- line_search(update, x, gx, g, on=True): the stored evaluation starts as (s = 0, phi0, g0)
    const float phi0 = ls_phi(ss), der = -phi0;
    float st_s = 0.f, st_phi = phi0;
    bool st_init = true;                                             // the stored evaluation is (x, gx) itself
    float* ft = nullptr;
    auto phi = [&](float sv, float& out) -> int {                   // :76-86
      if (sv == st_s) {
        out = st_phi;
        return INF_OK;
      }
      if (!(sv == 1.f && xt_full)) INF_TRY(launch_line_step(x, bf.upd, sv, xt, bf.dx, (long)E, s));
      xt_full = sv == 1.f;
      ft = pick(fpool, br.flow, fx);
      bf.fcur = ft;
      INF_TRY(resid(xt, gt, bf.dg, gx));                             // g, f and dg = g - g0 of the trial point
      INF_TRY(read_sumsq(f, B, bf, ss_t, s));
      out = ls_phi(ss_t);
      st_s = sv;
      st_phi = out;
      st_init = false;
      return INF_OK;
    };
    const float c1 = 1e-4f, amin = 1e-2f;
    float acc = 1.f;
    bool found = false;
    int ite = 0;
    float pa0;
    INF_TRY(phi(1.f, pa0));                                          // scalar_search_armijo (:24-63)
    if (pa0 <= phi0 + c1 * der) {
      found = true;
    } else {
      float a0 = 1.f;
      float a1 = -der * 1.f / 2.f / (pa0 - phi0 - der * a0);
      float pa1;
      INF_TRY(phi(a1, pa1));
      while (a1 > amin) {
        const float fac = a0 * a0 * (a1 * a1) * (a1 - a0);
        const float r1 = pa1 - phi0 - der * a1, r0 = pa0 - phi0 - der * a0;
        float a = a0 * a0 * r1 - a1 * a1 * r0;
        a = a / fac;
        float b = -(a0 * a0 * a0) * r1 + a1 * a1 * a1 * r0;
        b = b / fac;
        float a2 = (-b + sqrtf(fabsf(b * b - 3.f * a * der))) / (3.f * a);
        float pa2;
        INF_TRY(phi(a2, pa2));
        ite += 1;
        if (pa2 <= phi0 + c1 * a2 * der) {
          acc = a2;
          found = true;
          break;
        }
        if ((a1 - a2) > a1 / 2.f || (1.f - a2 / a1) < 0.96f) a2 = a1 / 2.f;
        a0 = a1;
        a1 = a2;
        pa0 = pa1;
        pa1 = pa2;
      }
    }
    if (!found) {                                                    // :90-92
      acc = 1.f;
      ite = 0;
    }
    if (acc != st_s) {                                               // :94-98 (a fresh evaluation at the step)
      st_s = acc + 1.f;                                              // (anything else: phi evaluates)
      float unused;
      INF_TRY(phi(acc, unused));
    } else if (st_init) {                                            // the accepted step is 0: x0 and g0 themselves
      INF_TRY(launch_line_step(x, bf.upd, 0.f, xt, bf.dx, (long)E, s));
      ft = pick(fpool, br.flow, fx);
      INF_HIP(hipMemcpyAsync(gt, gx, sizeof(float) * E, hipMemcpyDeviceToDevice, s));
      INF_HIP(hipMemsetAsync(bf.dg, 0, sizeof(float) * E, s));
      if (keep_f) INF_HIP(hipMemcpyAsync(ft, fx, sizeof(float) * E, hipMemcpyDeviceToDevice, s));
      ss_t = ss;
      xt_full = false;
    }
    // ---- the step is taken: x_est, g(x_est), delta_x (bf.dx), delta_g (bf.dg)
    x = xt;
    std::swap(gx, gt);
    fx = ft;
    ss = ss_t;
    nstep += 1;
    tnstep += ite + 1;                                               // :155-156
    obj = sqrt(total(ss));
    br.trace.push_back(obj);
    br.record(obj, nstep, x, keep_f ? fx : nullptr, ss);
    if (br.stop(obj, nstep) != Stop::GO) break;
    // the rank-1 update and update = -matvec(...) (:174-181); its x + update is the next search's s = 1 point
    xt = pick(xpool, br.low, x);
    INF_TRY(launch_broyden_update(br.update_args(nstep, x, gx, xt), s));
    xt_full = true;
  }
  br.write_trace();
  br.finish(nstep, tnstep);
  return INF_OK;
}

// f(0) for sample 0 of a conv net, computed once per (weights, batch size) with a B-sized launch
int ensure_f0(InfNet* f, int B, Bufs& bf, hipStream_t s) {
  if (f->f0_batch == B) return INF_OK;
  const size_t per = (size_t)f->d;
  if (!f->f0 && hipMalloc(&f->f0, per * sizeof(float)) != hipSuccess) return INF_ERR_HIP;
  INF_HIP(hipMemsetAsync(bf.zero, 0, sizeof(float) * per * B, s));
  OutArgs a;
  memset(&a, 0, sizeof(a));
  a.out0 = bf.fcur;
  INF_TRY(run_forward(f, bf.zero, B, bf, OM_PLAIN, &a, s));
  // sample 0's f(0): conv layout (B, d) row 0; fc layout (d, B) column 0
  if (f->fc)
    INF_HIP(hipMemcpy2DAsync(f->f0, sizeof(float), bf.fcur, sizeof(float) * (size_t)B, sizeof(float), per,
                             hipMemcpyDeviceToDevice, s));
  else
    INF_HIP(hipMemcpyAsync(f->f0, bf.fcur, per * sizeof(float), hipMemcpyDeviceToDevice, s));
  f->f0_batch = B;
  return INF_OK;
}

// find_fixed_point (implicit_block.py:17-28) of z <- x_embed - f(z) from z0 = y (internal layout):
//   x, x_prev = g(y), y; while not all((x - x_prev)^2 / (eps + eps |y|) < 1): x, x_prev = g(x), x; i += 1;
//   break once i > threshold.
// todo == nullptr: the reference's batch-wide test (torch.all over the batch), result for every sample in
// bf.lowest.  todo (host, B flags): the same loop per sample (a batch of one each, in lockstep launches); only
// the flagged samples' rows of bf.lowest are replaced.  *iters = the loop's i.
int banach_solve(InfNet* f, const float* y, int B, double eps_in, int threshold, const int* todo, Bufs& bf,
                 hipStream_t s, int* iters) {
  const size_t E = (size_t)B * f->d;
  const long sb = f->fc ? 1 : f->d, si = f->fc ? B : 1;
  float *zc = bf.xa, *zn = bf.xb;
  INF_HIP(hipMemsetAsync(bf.zero, 0, sizeof(float) * E, s));
  std::vector<double> dummy(B);
  int it = 0;
  // x = g(y), x_prev = y
  INF_TRY(eval_resid(f, y, bf.zero, bf.xemb, zc, nullptr, nullptr, B, bf, dummy, s));
  INF_HIP(hipMemcpyAsync(zn, y, sizeof(float) * E, hipMemcpyDeviceToDevice, s));
  if (!todo) {
    for (;;) {
      unsigned int bad = 0;
      INF_HIP(hipMemsetAsync(bf.counter, 0, sizeof(unsigned int), s));
      INF_TRY(glue_fixed_point_check(zc, zn, y, (long)E, (float)eps_in, bf.counter, s));
      INF_HIP(hipMemcpyAsync(&bad, bf.counter, sizeof(unsigned int), hipMemcpyDeviceToHost, s));
      INF_HIP(hipStreamSynchronize(s));
      if (bad == 0) break;
      INF_TRY(eval_resid(f, zc, bf.zero, bf.xemb, zn, nullptr, nullptr, B, bf, dummy, s));
      std::swap(zc, zn);
      it += 1;
      if (it > threshold) break;
    }
    INF_HIP(hipMemcpyAsync(bf.lowest, zc, sizeof(float) * E, hipMemcpyDeviceToDevice, s));
    *iters = it;
    return INF_OK;
  }
  std::vector<int> flags(todo, todo + B);
  INF_HIP(hipMemcpyAsync(bf.ps_improved, flags.data(), sizeof(int) * B, hipMemcpyHostToDevice, s));
  for (;;) {
    INF_TRY(launch_ps_fixed_point(zc, zn, y, bf.lowest, bf.ps_improved, B, f->d, sb, si, (float)eps_in, 0, s));
    INF_HIP(hipMemcpyAsync(flags.data(), bf.ps_improved, sizeof(int) * B, hipMemcpyDeviceToHost, s));
    INF_HIP(hipStreamSynchronize(s));
    bool any = false;
    for (int b = 0; b < B; ++b) any = any || flags[b];
    if (!any) break;
    INF_TRY(eval_resid(f, zc, bf.zero, bf.xemb, zn, nullptr, nullptr, B, bf, dummy, s));
    std::swap(zc, zn);
    it += 1;
    if (it > threshold) {      // the remaining samples take the latest iterate
      INF_TRY(launch_ps_fixed_point(zc, zn, y, bf.lowest, bf.ps_improved, B, f->d, sb, si, (float)eps_in, 1, s));
      break;
    }
  }
  *iters = it;
  return INF_OK;
}

// x_embed = e(y) + y, fx = e(y) (implicit_block.py:60,71) on yi = y in the internal layout (left in bf.xin)
int embed(InfNet* f, InfNet* e, const float* y, int B, Bufs& bf, const float** yi, hipStream_t s) {
  INF_TRY(to_internal(f, y, bf.xin, B, s, yi));
  OutArgs a;
  memset(&a, 0, sizeof(a));
  a.in0 = *yi;
  a.out0 = bf.fx;
  a.out1 = bf.xemb;
  return run_forward(e, *yi, B, bf, OM_EMBED, &a, s);
}

// the block kernel's readback buffer and event (fc_block_eval)
thread_local char* g_bk_host = nullptr;
thread_local size_t g_bk_host_cap = 0;
thread_local hipEvent_t g_bk_ev = nullptr;

}  // namespace

// Host wait on a readback event.  A blocking hipEventSynchronize that has to wait long (e.g. behind a whole
// log-det series) lets the runtime put the thread to sleep, and its wake-up comes late, with the GPU idle
// and nothing else queued; polling hipEventQuery keeps the host turnaround at the copy's latency.  The poll
// spins for at most 100 us, then yields the core between polls (other host threads, e.g. data loaders, run),
// and after 5 ms sleeps 20 us per poll.  INFLOW_BLOCKING_WAIT=1 restores the blocking wait.
int inf::host_wait(hipEvent_t ev) {
  static const bool blocking = [] {
    const char* e = getenv("INFLOW_BLOCKING_WAIT");
    return e && e[0] == '1';
  }();
  if (blocking) {
    INF_HIP(hipEventSynchronize(ev));
    return INF_OK;
  }
  const auto t0 = std::chrono::steady_clock::now();
  for (;;) {
    const hipError_t q = hipEventQuery(ev);
    if (q == hipSuccess) return INF_OK;
    if (q != hipErrorNotReady) {
      set_hip_error(q);
      return INF_ERR_HIP;
    }
    const auto us = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    if (us > 5000) std::this_thread::sleep_for(std::chrono::microseconds(20));
    else if (us > 100) std::this_thread::yield();
  }
}

InfBroydenStats inf::stats_for(const InfBroydenStats* caller) {
  InfBroydenStats st;
  memset(&st, 0, sizeof(st));
  if (caller) st = *caller;
  reset_stats(st);
  return st;
}

int inf::broyden_solve(InfNet* f, const float* y, int B, int T, double eps_in, InfBroydenStats* st, float* diff_detail,
                       Bufs& bf, hipStream_t s, SpecTail* tail) {
  InfBroydenStats stats = stats_for(st);
  std::vector<double> lowest_ss;
  INF_TRY(ensure_f0(f, B, bf, s));
  bool first = true;             // Broyden starts at z = 0 (broyden.py:136-144): f(0) is cached (per batch size, so
                                 // that it has the bits of the batch's own kernels)
  const ResidFn resid = [&](const float* x, float* gout, float* dg, const float* gprev) {
    if (first) {
      first = false;
      if (f->fc) return launch_resid_bcast_fc(f->f0, bf.xemb, x, gout, bf.fcur, bf.part, B, f->d, s);
      return launch_resid_bcast(f->f0, bf.xemb, x, gout, bf.fcur, bf.part, B, f->d, bf.nchunk, s, bf.sample_sums,
                                bf.stop_ev, &bf.stop_bound);
    }
    return eval_resid_part(f, x, x, bf.xemb, gout, dg, gprev, B, bf, s);
  };
  // fused fc nets: each later iteration's update and residual are one launch (fcnet.hip br_on)
  const StepFn step = [&](const BroydenArgs& ba, float* gout, float* dg, const float* gprev) {
    FcArgs fa = fc_args(f, ba.xnew, B);
    fa.o = resid_out(ba.xnew, bf.xemb, gout, dg, gprev, bf);   // (an fc net: bf.sample_sums is never set)
    fa.o.mode = OM_RESID;
    fa.o.bias = f->L.back().b;
    fa.br_on = 1;
    fa.br = ba;
    return launch_fcnet(fa, false, s);
  };
  const StartFn start = [&](float* x0, float* g0, float* upd, float* x1, float* dx) {
    first = false;
    if (!f->fc)          // (conv: broyden_core's zero-copy per-sample sums are on whenever this start is passed)
      return launch_broyden_start_sample(f->f0, bf.xemb, x0, g0, bf.fcur, bf.part, bf.stop_ev, &bf.stop_bound, upd,
                                         x1, dx, B, f->d, s);
    return launch_broyden_start_fc(f->f0, bf.xemb, x0, g0, bf.fcur, bf.part, bf.stop_ev, &bf.stop_bound, upd, x1, dx,
                                   B, f->d, s);
  };
  // conv nets: the one-launch start where the residual sums go straight into the readback slot (broyden_core zc)
  const bool conv_start = !f->fc && out_nchunk(f->d) <= 4;
  if (f->line_search) {
    // line_search(on=True) (broyden.py:66-99): the global rule only (a per-sample step size is not the reference's)
    if (f->convergence != INF_CONV_GLOBAL) return INF_ERR_UNSUPPORTED;
    INF_TRY(broyden_core_ls(f, resid, B, T, eps_in, stats, lowest_ss, bf, s, /*keep_f=*/true));
  } else {
    INF_TRY(broyden_core(f, resid, B, T, eps_in, stats, lowest_ss, bf, s, /*keep_f=*/true, f->fcfused ? &step : nullptr,
                         ((f->fc && f->d <= FC_NARROW_MAX) || conv_start) ? &start : nullptr, tail,
                         /*resid_sample_sums=*/true));
  }
  if (diff_detail) {
    std::vector<float> dd(B);
    for (int b = 0; b < B; ++b) dd[b] = (float)sqrt(lowest_ss[b]);
    INF_HIP(hipMemcpyAsync(diff_detail, dd.data(), sizeof(float) * B, hipMemcpyHostToDevice, s));
    INF_HIP(hipStreamSynchronize(s));
  }
  if (stats.prot_break) {
    // banach_find_root (implicit_block.py:57-65,74-75): z <- x_embed - f(z) from z0 = y, <= 1000 iterations;
    // per-sample mode: only the samples whose own solve broke, each with its own stopping test
    std::vector<int> todo;
    if (f->convergence == INF_CONV_PER_SAMPLE) {
      const int stride = PS_HEAD + T;
      std::vector<double> pst((size_t)B * stride);
      INF_HIP(hipMemcpyAsync(pst.data(), bf.ps_state, sizeof(double) * pst.size(), hipMemcpyDeviceToHost, s));
      INF_HIP(hipStreamSynchronize(s));
      todo.resize(B);
      for (int b = 0; b < B; ++b) todo[b] = (int)pst[(size_t)b * stride + 5];
    }
    int it = 0;
    INF_TRY(banach_solve(f, y, B, eps_in, 1000, todo.empty() ? nullptr : todo.data(), bf, s, &it));
    stats.fixed_point_iters = it;
  }
  if (st) *st = stats;
  return INF_OK;
}

// inf_imblock_eval_exact on the device-resident block kernel (fcblock.hip): one launch, one readback of its
// statistics; a protective break runs the Banach fallback and the recompute on the host path (as below).
int inf::fc_block_eval(InfNet* nx, InfNet* nz, const float* x, float* z, float* logdet_x, float* logdet_z, int B, int T,
                       double eps_in, InfBroydenStats* stats, Bufs& bf, hipStream_t s) {
  if (nx->mfma_mode != INF_MFMA_F16X3 || nz->mfma_mode != INF_MFMA_F16X3 || !bf.bk_sync || nz->line_search)
    return INF_ERR_UNSUPPORTED;
  FcBlockArgs a;
  memset(&a, 0, sizeof(a));
  a.nx = fc_args(nx, nullptr, B);
  a.nz = fc_args(nz, nullptr, B);
  a.B = B;
  a.T = T;
  a.per_sample = nz->convergence == INF_CONV_PER_SAMPLE;
  if (!fcblock_supported(a)) return INF_ERR_UNSUPPORTED;
  const int d = nz->d;
  a.eps = eps_in * sqrt((double)B * d);                              // broyden.py:131
  a.eps_ps = eps_in * sqrt((double)d);
  a.x = x;
  a.z = z;
  a.logdet_x = logdet_x;
  a.logdet_z = logdet_z;
  a.xin_g = bf.xin;
  a.fx_g = bf.fx;
  a.xemb_g = bf.xemb;
  a.lowx_g = bf.lowest;
  a.lowf_g = bf.flow;
  a.error = bf.bk_sync;
  a.gran = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(bf.bk_sync) + 16);
  a.tag0 = 1;
  FcBlockStats* dst = reinterpret_cast<FcBlockStats*>(bf.bk_out);
  a.stats = dst;
  a.s_nstep = reinterpret_cast<int*>(bf.bk_out + sizeof(FcBlockStats));
  a.s_lstep = a.s_nstep + B;
  a.s_prot = a.s_lstep + B;
  a.s_lowest = reinterpret_cast<double*>(bf.bk_out + ((sizeof(FcBlockStats) + sizeof(int) * 3 * (size_t)B + 7) & ~(size_t)7));
  INF_HIP(hipMemsetAsync(bf.bk_sync, 0, bf.bk_sync_bytes, s));
  INF_TRY(launch_fcblock(a, s));
  // one readback: the error word and the statistics (per-sample rule: the per-sample arrays too)
  const size_t nbytes = a.per_sample ? bf.bk_out_bytes : sizeof(FcBlockStats);
  if (g_bk_host_cap < nbytes + 16) {
    if (g_bk_host) (void)hipHostFree(g_bk_host);
    g_bk_host = nullptr;
    g_bk_host_cap = 0;
    if (hipHostMalloc(reinterpret_cast<void**>(&g_bk_host), nbytes + 16, hipHostMallocCoherent) != hipSuccess)
      return INF_ERR_HIP;
    g_bk_host_cap = nbytes + 16;
  }
  INF_HIP(hipMemcpyAsync(g_bk_host, bf.bk_sync, 16, hipMemcpyDeviceToHost, s));
  INF_HIP(hipMemcpyAsync(g_bk_host + 16, bf.bk_out, nbytes, hipMemcpyDeviceToHost, s));
  if (!g_bk_ev && hipEventCreateWithFlags(&g_bk_ev, INF_EV_SYNC) != hipSuccess) return INF_ERR_HIP;
  hipEvent_t ev = g_bk_ev;
  INF_HIP(hipEventRecord(ev, s));
  INF_TRY(host_wait(ev));
  if (*reinterpret_cast<unsigned*>(g_bk_host) != 0) {
    set_hip_error(hipErrorLaunchTimeOut);
    return INF_ERR_HIP;
  }
  const FcBlockStats* hs = reinterpret_cast<const FcBlockStats*>(g_bk_host + 16);
  InfBroydenStats st = stats_for(stats);
  st.convergence = nz->convergence;
  if (!a.per_sample) {
    st.nstep = hs->nstep;
    st.lowest_step = hs->lowest_step;
    st.prot_break = hs->prot_break;
    st.n_trace = std::min(hs->n_trace, 64);
    for (int k = 0; k < st.n_trace; ++k) st.trace[k] = hs->trace[k];
    st.diff = hs->lowest;
    st.eps = a.eps;
  } else {
    const char* base = g_bk_host + 16;
    const int* sn = reinterpret_cast<const int*>(base + sizeof(FcBlockStats));
    const int* sl = sn + B;
    const int* sp = sl + B;
    const double* slo = reinterpret_cast<const double*>(
        base + ((sizeof(FcBlockStats) + sizeof(int) * 3 * (size_t)B + 7) & ~(size_t)7));
    double d2 = 0.0;
    for (int b = 0; b < B; ++b) {
      st.nstep = std::max(st.nstep, sn[b]);
      st.lowest_step = std::max(st.lowest_step, sl[b]);
      st.prot_break |= sp[b];
      d2 += slo[b] * slo[b];
      if (st.sample_nstep) st.sample_nstep[b] = sn[b];
      if (st.sample_lowest_step) st.sample_lowest_step[b] = sl[b];
      if (st.sample_prot_break) st.sample_prot_break[b] = sp[b];
    }
    st.diff = sqrt(d2);
    st.eps = a.eps_ps;
  }
  st.tnstep = st.nstep;
  if (st.prot_break) {
    // banach_find_root (implicit_block.py:57-65,74-75) from z0 = x, as broyden_solve does, on the buffers the kernel
    // left: x_embed, f_x(x), x and the lowest iterates (per-sample rule: only the samples whose own solve broke)
    std::vector<int> todo;
    if (a.per_sample) {
      const int* sp = reinterpret_cast<const int*>(g_bk_host + 16 + sizeof(FcBlockStats)) + 2 * B;
      todo.assign(sp, sp + B);
    }
    int it = 0;
    INF_TRY(banach_solve(nz, bf.xin, B, eps_in, 1000, todo.empty() ? nullptr : todo.data(), bf, s, &it));
    st.fixed_point_iters = it;
    OutArgs o;
    memset(&o, 0, sizeof(o));
    o.in0 = bf.fx;
    o.in1 = bf.xin;
    o.out0 = bf.tmp;
    INF_TRY(run_forward(nz, bf.lowest, B, bf, OM_RECOMP, &o, s));
    FcArgs fjz = fc_args(nz, bf.tmp, B);
    fjz.logdet = logdet_z;
    INF_TRY(launch_fcnet(fjz, true, s));
    INF_TRY(to_boundary(nx, bf.tmp, z, B, s));
  }
  if (stats) *stats = st;
  return INF_OK;
}

void inf::solve_release_thread() {
  for (SumsSlot& sl : g_sums_slots) {
    if (sl.host) (void)hipHostFree(sl.host);
    if (sl.ev) (void)hipEventDestroy(sl.ev);
    sl = SumsSlot{};
  }
  if (g_bk_host) (void)hipHostFree(g_bk_host);
  g_bk_host = nullptr;
  g_bk_host_cap = 0;
  if (g_bk_ev) (void)hipEventDestroy(g_bk_ev);
  g_bk_ev = nullptr;
}

extern "C" {

int inf_root_find(InfNet* f, InfNet* e, const float* y, float* out, int B, int T, double eps, InfBroydenStats* stats,
                  float* diff_detail, void* ws, size_t ws_bytes, void* stream) {
  if (!f || !e || !y || !out || B <= 0 || T <= 0 || T > 64 || !same_shape(f, e)) return INF_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  Bufs bf;
  INF_TRY(carve_ws(f, B, T, ws, ws_bytes, bf));
  const float* yi;
  INF_TRY(embed(f, e, y, B, bf, &yi, s));
  INF_TRY(broyden_solve(f, yi, B, T, eps, stats, diff_detail, bf, s));
  return to_boundary(f, bf.lowest, out, B, s);
}

int inf_imblock_forward(InfNet* nx, InfNet* nz, const float* x, float* z, int B, int T, double eps,
                        InfBroydenStats* stats, void* ws, size_t ws_bytes, void* stream) {
  if (!nx || !nz || !x || !z || B <= 0 || T <= 0 || T > 64 || !same_shape(nx, nz)) return INF_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  Bufs bf;
  INF_TRY(carve_ws(nx, B, T, ws, ws_bytes, bf));
  const float* xi;
  InfBroydenStats st = stats_for(stats);
  INF_TRY(embed(nz, nx, x, B, bf, &xi, s));
  INF_TRY(broyden_solve(nz, xi, B, T, eps, &st, nullptr, bf, s));
  if (stats) *stats = st;
  // z = (nnet_x(x) - nnet_z(z*)) + x   (implicit_block.py:227).  nnet_z(z*) was evaluated by the residual
  // that produced the lowest iterate (same input, same kernel: the same bits) and kept in bf.flow; only
  // after the Banach fallback (prot_break) is it evaluated again.
  return write_boundary(nx, bf, z, B, s, [&](float* o) {
    if (!st.prot_break) return glue_recomp(bf.fx, bf.flow, xi, o, (long)B * nx->d, s);
    OutArgs a;
    memset(&a, 0, sizeof(a));
    a.in0 = bf.fx;
    a.in1 = xi;
    a.out0 = o;
    return run_forward(nz, bf.lowest, B, bf, OM_RECOMP, &a, s);
  });
}

// Implicit backward of an imBlock (imBlock.Backward.backward, implicit_block.py:176-217):
//   dl_dh: Broyden root of g(y) = y (I + J_fz(z)) - grad from y = 0 (eps_backward, threshold), lowest iterate;
//   dl_dx = dl_dh (I + J_fx(x)).
int inf_imblock_backward(InfNet* nx, InfNet* nz, const float* z, const float* x, const float* grad, float* dl_dh,
                         float* dl_dx, int B, int T, double eps, InfBroydenStats* stats, void* ws, size_t ws_bytes,
                         void* stream) {
  if (!nx || !nz || !z || !x || !grad || !dl_dh || !dl_dx || B <= 0 || T <= 0 || T > 64 || !same_shape(nx, nz))
    return INF_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  {
    Bufs bf;
    INF_TRY(carve_ws(nz, B, T, ws, ws_bytes, bf));
    const float *zi, *gi;
    INF_TRY(to_internal(nz, z, bf.xin, B, s, &zi));
    INF_TRY(to_internal(nz, grad, bf.xemb, B, s, &gi));
    INF_TRY(run_forward(nz, zi, B, bf, -1, nullptr, s));      // activation derivatives at z
    InfBroydenStats bs = stats_for(stats);
    std::vector<double> lowest_ss;
    const ResidFn resid = [&](const float* y, float* gout, float* dg, const float* gprev) {
      return vjp_resid_part(nz, y, zi, gi, gout, dg, gprev, B, bf, s);
    };
    INF_TRY(broyden_core(nz, resid, B, T, eps, bs, lowest_ss, bf, s));
    if (stats) *stats = bs;
    INF_TRY(to_boundary(nz, bf.lowest, dl_dh, B, s));
  }
  // dl_dx = dl_dh + dl_dh^T J_fx(x)   (Fx = nnet_x(x) + x; Fx.backward(dl_dh), :210-213)
  Bufs bf;
  INF_TRY(carve_ws(nx, B, 1, ws, ws_bytes, bf));
  const float *xi, *hi;
  INF_TRY(to_internal(nx, x, bf.xin, B, s, &xi));
  INF_TRY(to_internal(nx, dl_dh, bf.eps_t, B, s, &hi));
  INF_TRY(run_forward(nx, xi, B, bf, -1, nullptr, s));
  INF_TRY(run_vjp(nx, hi, bf.va, xi, nullptr, nullptr, B, bf, s));
  return write_boundary(nx, bf, dl_dx, B, s,
                        [&](float* o) { return glue_add(bf.va, hi, o, (long)B * nx->d, s); });
}

int inf_banach_find_root(InfNet* f, InfNet* e, const float* y, float* out, int B, int threshold, double eps,
                         int* iters, void* ws, size_t ws_bytes, void* stream) {
  if (!f || !e || !y || !out || B <= 0 || threshold < 0 || !same_shape(f, e)) return INF_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  Bufs bf;
  INF_TRY(carve_ws(f, B, 1, ws, ws_bytes, bf));
  const float* yi;
  INF_TRY(embed(f, e, y, B, bf, &yi, s));
  std::vector<int> todo;
  if (f->convergence == INF_CONV_PER_SAMPLE) todo.assign(B, 1);
  int it = 0;
  INF_TRY(banach_solve(f, yi, B, eps, threshold, todo.empty() ? nullptr : todo.data(), bf, s, &it));
  if (iters) *iters = it;
  return to_boundary(f, bf.lowest, out, B, s);
}

size_t inf_broyden_workspace_bytes(int batch, int d, int threshold) {
  const size_t nchunk = (size_t)(d + 1023) / 1024;
  return sizeof(double) * ((size_t)batch * nchunk * (3 * (size_t)threshold + 2) + 64);
}

int inf_broyden_update(float* U, float* VT, const float* dx, const float* dg, const float* gx, const float* x,
                       float* update, float* x_next, float* dx_next, int B, int d, int T, int nstep, void* ws,
                       size_t ws_bytes, void* stream) {
  if (!U || !VT || !dx || !dg || !gx || !x || !update || !x_next || !dx_next || B <= 0 || d <= 0 || T <= 0 ||
      T > 64 || nstep < 1 || nstep > T)
    return INF_ERR_INVALID;
  if (!ws || ws_bytes < inf_broyden_workspace_bytes(B, d, T)) return INF_ERR_WORKSPACE;
  BroydenArgs ba;
  memset(&ba, 0, sizeof(ba));
  ba.batch = B;
  ba.d = d;
  ba.T = T;
  ba.sb = d;
  ba.si = 1;
  ba.cs = (long)B * d;
  ba.U = U;
  ba.VT = VT;
  ba.dx = dx;
  ba.dg = dg;
  ba.gx = gx;
  ba.x = x;
  ba.xnew = x_next;
  ba.dxnew = dx_next;
  ba.upd = update;
  ba.part = reinterpret_cast<double*>(ws);
  ba.m = (nstep - 1) % T;
  ba.ncols = std::min(nstep, T);
  return launch_broyden_update(ba, (hipStream_t)stream);
}

int inf_broyden_line_step(const float* x0, const float* update, float step, float* x_est, float* dx, size_t n,
                          void* stream) {
  if (!x0 || !update || !x_est || !dx || n == 0) return INF_ERR_INVALID;
  return launch_line_step(x0, update, step, x_est, dx, (long)n, (hipStream_t)stream);
}

}  // extern "C"
