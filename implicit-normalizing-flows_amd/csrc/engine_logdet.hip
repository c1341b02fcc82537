// The log-det estimators and the eval schedules built on them: the fused nets' power series (one launch per term for
// one or two nets), the side stream of the overlapped eval pass, the fc eval pass and its chain over blocks, and the
// series / Neumann / exact / trace entries.
//
// Reference mapping (implicit_block.py unless noted):
//   inf_imblock_eval            <- imBlock.forward + _logdetgrad in eval                 (:220-234, 245-322)
//   inf_imblock_eval_exact      <- the same with brute_force=True                        (:249-260, 358-362)
//   inf_flow_eval_exact_chain   <- SequentialFlow over fc imBlocks (container.py:12-20; train_tabular.py:314-336)
//   inf_logdet_series[_pair]    <- basic_logdet_estimator                                (:418-426)
//   inf_neumann_vector[_pair]   <- neumann_logdet_estimator's vjp loop                   (:429-436)
//   inf_logdet_neumann          <- neumann_logdet_estimator                              (:429-438)
//   inf_logdet_exact            <- brute-force batch_jacobian + torch.logdet             (:249-260)
//   inf_logdet_exact_trace      <- exact_trace=True                                      (:323-343)
#include "engine.h"

using namespace inf;

namespace {

// whether both nets of a series launch carry the f16x3 operands
bool series_h3(const InfNet* a, const InfNet* b) {
  return a->mfma_mode == INF_MFMA_F16X3 && b->mfma_mode == INF_MFMA_F16X3;
}
// The kernel family of a series term's VJP launch over `nnets` nets (a: the first, whose policy the launch follows;
// b: the last), as launch_net313_multi decides it
int series_family(const InfNet* a, const InfNet* b, int B, int nnets) {
  return net313_family(a->fhid, a->C, a->H, a->W, B, nnets, nnets, a->k128, MODE_VJP, series_h3(a, b));
}

// Power series of 1 or 2 fused nets of the same shape (the x- and z-branch of an imBlock advance in
// lockstep: one launch per term over both nets' tiles).  Term k's VJP stages term k-1's packed taps
// directly (tap sum, preact swish', trace partial -- conv_out's work), so a term is ONE launch; only
// the last term's taps go through conv_out.  Series slabs: part[k][b][snchunk] (zeroed first: the
// fused kernel fills one entry per tile, conv_out one per 1024-element chunk).
// Neumann mode (wouts != nullptr, ncoeff a host array of n_terms + 1): instead of the trace partials, each
// term's staging accumulates w += ncoeff[k] v_k for its own pixels (w starts as eps, the last term's taps go
// through conv_out), i.e. the Neumann vector of implicit_block.py:430-436 for 1 or 2 nets in lockstep.
//
// Sample groups (INF_OPT_SERIES_GROUP): the series is independent per sample (the 3x3 halo never crosses
// an image), so it runs as one complete chain per group of G samples, a group's derivative-saving forward directly in
// front of its terms: the d1 / d2 planes live between two terms, read again by every term, are then a group's and not
// the whole batch's (the rule sizes a group to the memory-side cache).  A group's buffers are the batch's own, sliced
// by pointer: every per-sample buffer moves by the group's first sample (the pair layout included: each net's planes are its own buffer, indexed by the net's own
// tiles), the trace slab's base too while its term stride stays B x snchunk.  Each group launches on the whole batch's
// kernel family and its tiles do the whole batch's arithmetic: bitwise the same results for every G.  The closing
// conv_out / combine launches stay one over the whole batch.  concurrent: the series running side by side with this one
// included (inf_imblock_eval's overlapped schedule: 2).
int series_fused(InfNet* const* nets, const float* const* xs, const float* const* es, int nn, const float* coeff,
                 int n_terms, float* const* outs, int B, Bufs* bfs, hipStream_t s, unsigned save_mask = 3u,
                 float* const* wouts = nullptr, const float* ncoeff = nullptr, int concurrent = 1) {
  const InfNet* n0 = nets[0];
  const int fam = series_family(n0, nets[nn - 1], B, nn);
  if (fam < 0) return INF_ERR_UNSUPPORTED;
  for (int i = 0; i < nn; ++i) {
    if (!wouts) INF_HIP(hipMemsetAsync(bfs[i].part, 0, sizeof(double) * n_terms * B * bfs[i].snchunk, s));
    else INF_HIP(hipMemcpyAsync(wouts[i], es[i], sizeof(float) * (size_t)B * nets[i]->d, hipMemcpyDeviceToDevice, s));
  }
  const int G = n0->series_group > 0 ? std::min(n0->series_group, B)
                                     : net313_series_group(n0->fhid, n0->C, n0->H, n0->W, B, nn, concurrent, n0->k128,
                                                           series_h3(n0, nets[nn - 1]));
  // per-sample strides of the sliced buffers: d1 / d2 in the family's tile layout, the packed taps, the vectors
  const size_t dstr = net313_dstride(n0->fhid, n0->H, n0->W, fam), ystr = (size_t)n0->M3 * n0->P, vstr = (size_t)n0->d;
  const unsigned all = (1u << nn) - 1u;
  Net313Args args[2];
  for (int g0 = 0; g0 < B; g0 += G) {
    const int Bg = std::min(G, B - g0);
    auto group_args = [&](int i, const float* in, bool vjp) {
      Net313Args v = net313_args(nets[i], in + g0 * vstr, Bg, bfs[i], vjp);
      v.d1 += g0 * dstr;
      v.d2 += g0 * dstr;
      v.Y += g0 * ystr;
      return v;
    };
    // activation derivatives (in the pair's tile layout); a net whose d1/d2 are already saved is skipped
    for (int i = 0; i < nn; ++i) args[i] = group_args(i, xs[i], false);
    if ((save_mask & all) == all) {
      INF_TRY(launch_net313_multi(args, nn, n0->fhid, MODE_SAVE, s, 0, B));
    } else {
      for (int i = 0; i < nn; ++i)
        if (save_mask & (1u << i)) INF_TRY(launch_net313_multi(&args[i], 1, n0->fhid, MODE_SAVE, s, nn, B));
    }
    for (int k = 0; k < n_terms; ++k) {
      for (int i = 0; i < nn; ++i) {
        InfNet* n = nets[i];
        Bufs& bf = bfs[i];
        Net313Args& v = args[i];
        v = group_args(i, es[i], true);
        v.Y = ((k % 2 == 0) ? bf.Y : bf.Y2) + g0 * ystr;
        // serpentine: odd terms walk the tiles backwards, so a term starts on the derivative tiles the previous
        // one read last (still in the memory-side cache: s0 pair 349 -> 338 us per term)
        v.tile_order = k & 1;
        if (k > 0) {
          v.in = nullptr;
          v.in_taps = ((k % 2 == 1) ? bf.Y : bf.Y2) + g0 * ystr;
          v.vmul_x = n->pre_act != ACT_NONE ? xs[i] + g0 * vstr : nullptr;
          v.vmul_beta = n->pre_beta;
          v.vmul_act = n->pre_act == ACT_SWISH ? 0 : n->pre_act;
          if (wouts) {
            v.acc_w = wouts[i] + g0 * vstr;
            v.acc_coef = ncoeff[k];
          } else {
            v.dot_eps = es[i] + g0 * vstr;
            v.dot_part = bf.part + ((size_t)(k - 1) * B + g0) * bf.snchunk;
            v.dot_nchunk = bf.snchunk;
          }
        }
      }
      INF_TRY(launch_net313_multi(args, nn, n0->fhid, MODE_VJP, s, 0, B));
    }
  }
  // the last term's taps through conv_out: its trace partial, or (Neumann) its vector added to w
  for (int i = 0; i < nn; ++i) {
    InfNet* n = nets[i];
    Bufs& bf = bfs[i];
    OutArgs a;
    memset(&a, 0, sizeof(a));
    a.in0 = wouts ? nullptr : es[i];
    a.in1 = xs[i];
    a.out0 = bf.va;
    a.pre_beta = n->pre_beta;
    a.pre_act = n->pre_act;
    a.partial = wouts ? nullptr : bf.part + (size_t)(n_terms - 1) * B * bf.snchunk;
    a.nchunk = bf.snchunk;
    INF_TRY(out_stage(n, fused_taps(n), OM_VJP, a, ((n_terms - 1) % 2 == 0) ? bf.Y : bf.Y2, B, s));
    if (wouts) INF_TRY(glue_axpy_scaled(wouts[i], bf.va, ncoeff[n_terms], (long)B * n->d, s));
  }
  if (wouts) return INF_OK;
  for (int i = 0; i < nn; ++i)
    INF_TRY(launch_series_combine(bfs[i].part, coeff, n_terms, B, bfs[i].snchunk, outs[i], s));
  return INF_OK;
}

// One non-blocking side stream (+ fork / join events) per host thread and device, created on first use
// and kept for the process lifetime (calls on one thread are serial, so it is never shared concurrently).
struct SideStream {
  hipStream_t s = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
};
thread_local SideStream g_side[16];
SideStream* side_stream() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
  SideStream& ss = g_side[dev];
  if (!ss.s) {
    if (hipStreamCreateWithFlags(&ss.s, hipStreamNonBlocking) != hipSuccess) return nullptr;
    if (hipEventCreateWithFlags(&ss.fork, INF_EV_SYNC) != hipSuccess ||
        hipEventCreateWithFlags(&ss.join, INF_EV_SYNC) != hipSuccess)
      return nullptr;
  }
  return &ss;
}

// Joins the side stream into the caller's stream when the eval pass returns, on every path after the fork
// (an error return included): the caller's next call may reuse the workspace the side stream still uses.
struct SideJoin {
  SideStream* side = nullptr;
  hipStream_t s = nullptr;
  ~SideJoin() {
    if (!side) return;
    (void)hipEventRecord(side->join, side->s);
    (void)hipStreamWaitEvent(s, side->join, 0);
  }
};

// The next block's x-branch folded into this block's z-branch Jacobian launch (the chain call): both evaluate their net
// at this block's z, so one grid holds the two (launch_fcnet_jac_pair: 2 x 625 workgroups at B = 10 000 take 85 us
// against 2 x 56 us as two launches).  bf: the next block's buffers (its xin / fx / xemb), logdet: its
// logdet_x; done: the last launch this block queued was the pair (else the next block runs its own x-branch launch).
struct FcNextX {
  InfNet* nx = nullptr;
  Bufs* bf = nullptr;
  float* logdet = nullptr;
  bool done = false;
};
// The block's log-density step lout = lin - (logdet_x - logdet_z) folded into its z-branch Jacobian launch (the chain
// call); done: the last launch this block queued wrote it (else the caller runs glue_logp_step)
struct FcLogpStep {
  const float* lin = nullptr;
  float* lout = nullptr;
  bool done = false;
};
// whether inf_imblock_eval_exact takes the block kernel (fcblock.hip) for this solved net
bool fc_block_first(const InfNet* nz) {
  return nz->fc_block == 2 || (nz->fc_block == 1 && nz->convergence == INF_CONV_PER_SAMPLE);
}
// f16x3 planes on both nets of a pair launch, same shape
bool fc_pair_ok(const InfNet* a, const InfNet* b) {
  return a->fcfused && b->fcfused && a->mfma_mode == INF_MFMA_F16X3 && b->mfma_mode == INF_MFMA_F16X3 &&
         same_shape(a, b) && !a->L.empty() && !b->L.empty() && a->L[0].act == b->L[0].act;
}

// inf_imblock_eval_exact on carved buffers.  x_done: bf's xin / fx / xemb and logdet_x hold this block's x-branch
// already (the previous block's pair launch); next (nullable): fold the next block's x-branch into the z-branch launch.
int eval_exact_fc(InfNet* nx, InfNet* nz, const float* x, float* z, float* logdet_x, float* logdet_z, int B, int T,
                  double eps, InfBroydenStats* stats, Bufs& bf, hipStream_t s, bool x_done, FcNextX* next,
                  FcLogpStep* lp = nullptr) {
  if (next) next->done = false;
  if (lp) lp->done = false;
  // x in the internal layout: written by the x-branch JAC launch's staging (it reads x in the boundary layout)
  const float* xi = bf.xin;
  if (fc_block_first(nz)) {
    // the whole block in one launch (fcblock.hip); falls through to the launch-per-iteration path below when the
    // configuration has no block kernel or (global rule) its grid cannot be co-resident.  The default (1) takes it for
    // the per-sample rule only: under the global rule the launch path is faster
    const int st = fc_block_eval(nx, nz, x, z, logdet_x, logdet_z, B, T, eps, stats, bf, s);
    if (st != INF_ERR_UNSUPPORTED) return st;
  }
  // log|det(I + J_fx(x))| (implicit_block.py:358-362) and x_embed = f_x(x) + x (:71) in one launch: the JAC kernel's primal
  // column is f_x(x) with the FWD kernel's bits (the same 16-column tiles, k slices and partial order), so the x_embed
  // launch is folded into it.  (Run beside the root solve on the side stream instead, the JAC launch took every CU
  // first and the x_embed launch waited behind it anyway)  Then the root solve and
  // z = (f_x(x) - f_z(z*)) + x   (implicit_block.py:74-80, 227)
  if (!x_done) {
    FcArgs fjx = fc_args(nx, nullptr, B);
    fjx.x_bnd = x;
    fjx.x_int = bf.xin;
    fjx.logdet = logdet_x;
    fjx.o.in0 = xi;
    fjx.o.out0 = bf.fx;
    fjx.o.out1 = bf.xemb;
    INF_TRY(launch_fcnet(fjx, true, s));
  }
  // z = (f_x(x) - f_z(z*)) + x computed in the staging of the log|det(I + J_fz(z))| launch, which also writes z in the
  // boundary layout (the recompute and transpose launches of the path below, in one).  The solve queues it on its
  // predicted last iterate before it reads that iterate's norm (SpecTail), so the GPU does not wait for the host's
  // stop decision; if the solve's result is another iterate (or it breaks), it is queued again on the result.  With
  // next, the same launch evaluates the next block's x-branch at that z (its input recomputed in its own staging).
  auto jac_z = [&](const float* flow) {
    FcArgs fjz = fc_args(nz, nullptr, B);
    fjz.logdet = logdet_z;
    fjz.rc_fx = bf.fx;
    fjz.rc_fz = flow;
    fjz.rc_x = xi;
    fjz.rc_out = z;
    if (lp) {
      fjz.lp_in = lp->lin;
      fjz.lp_ldx = logdet_x;
      fjz.lp_out = lp->lout;
      lp->done = true;
    }
    if (next) {
      FcArgs fjn = fc_args(next->nx, nullptr, B);
      fjn.rc_fx = bf.fx;
      fjn.rc_fz = flow;
      fjn.rc_x = xi;
      fjn.x_int = next->bf->xin;
      fjn.logdet = next->logdet;
      fjn.o.out0 = next->bf->fx;
      fjn.o.out1 = next->bf->xemb;
      const int st = launch_fcnet_jac_pair(fjz, fjn, s);
      next->done = st == INF_OK;
      if (st != INF_ERR_UNSUPPORTED) return st;
    }
    return launch_fcnet(fjz, true, s);
  };
  SpecTail tail;
  tail.fn = [&](const float*, const float* f) { return jac_z(f); };
  InfBroydenStats sst = stats_for(stats);
  INF_TRY(broyden_solve(nz, xi, B, T, eps, &sst, nullptr, bf, s, nz->convergence == INF_CONV_GLOBAL ? &tail : nullptr));
  if (stats) *stats = sst;
  if (!sst.prot_break) {
    if (tail.x && tail.x == bf.lowest && tail.f == bf.flow) return INF_OK;   // the speculative launch has the result
    return jac_z(bf.flow);
  }
  if (next) next->done = false;
  if (lp) lp->done = false;
  OutArgs a;
  memset(&a, 0, sizeof(a));
  a.in0 = bf.fx;
  a.in1 = xi;
  a.out0 = bf.tmp;
  INF_TRY(run_forward(nz, bf.lowest, B, bf, OM_RECOMP, &a, s));
  // log|det(I + J_fz(z))| at the recomputed z
  FcArgs fjz = fc_args(nz, bf.tmp, B);
  fjz.logdet = logdet_z;
  INF_TRY(launch_fcnet(fjz, true, s));
  return to_boundary(nx, bf.tmp, z, B, s);
}

int eval_exact_check(InfNet* nx, InfNet* nz, const float* x, int B) {
  if (!nx->fcfused || !nz->fcfused || nx->d > 10) return INF_ERR_UNSUPPORTED;
  FcArgs probe = fc_args(nx, x, B);
  FcArgs probe_z = fc_args(nz, x, B);
  if (!fcnet_supported(probe, true) || !fcnet_supported(probe_z, true)) return INF_ERR_UNSUPPORTED;
  return INF_OK;
}

// The power series of fused f16x3 fc nets in one launch for the pair (fcblock.hip fcseries_kernel; inputs in the
// boundary layout), when the first net's INF_OPT_FC_SERIES is 1 and a kernel exists for the shape; else
// INF_ERR_UNSUPPORTED and the caller takes the per-layer path
int fc_series(InfNet* const* nets, const float* const* xs, const float* const* es, const float* coeff, int n_terms,
              float* const* outs, int nn, int B, hipStream_t s) {
  if (!nets[0]->fc_series || n_terms < 1) return INF_ERR_UNSUPPORTED;
  for (int i = 0; i < nn; ++i)
    if (!nets[i]->fcfused || !nets[i]->fcht || nets[i]->mfma_mode != INF_MFMA_F16X3) return INF_ERR_UNSUPPORTED;
  FcSeriesArgs a;
  memset(&a, 0, sizeof(a));
  a.nn = nn;
  a.nl = (int)nets[0]->L.size();
  a.d = nets[0]->d;
  a.act = nets[0]->L[0].act;
  a.B = B;
  a.n_terms = n_terms;
  for (int k = 0; k < n_terms; ++k) a.coeff[k] = coeff[k];
  for (int i = 0; i < nn; ++i) {
    const InfNet* n = nets[i];
    if ((int)n->L.size() != a.nl || n->d != a.d || n->L[0].act != a.act || a.nl > FC_MAXL) return INF_ERR_UNSUPPORTED;
    for (int l = 0; l < a.nl; ++l) {
      FcLayer& f = a.f[i].L[l];
      f.A = n->L[l].f.A;
      f.Ah = n->fch + n->fch_off[l];
      f.Aexp = n->fchexp + l;
      f.Kpad = n->L[l].f.Kpad;
      f.b = n->L[l].b;
      f.beta = n->L[l].act_beta;
      FcLayer& t = a.t[i].L[l];
      t.A = n->L[a.nl - 1 - l].g.A;                 // W_{nl-1-l}^T fp32 (the input layer's exact contraction)
      t.Kpad = n->L[a.nl - 1 - l].g.Kpad;
      t.Ah = n->fcht + n->fch_off[l];
      t.Aexp = n->fchtexp + l;
    }
    a.x[i] = xs[i];
    a.eps[i] = es[i];
    a.out[i] = outs[i];
  }
  return launch_fcseries(a, s);
}

// try_fc: the one-launch fc series first (inf_logdet_series); the pair's per-net fallback has already asked the first net
int series_single(InfNet* n, const float* x, const float* vareps, const float* coeff, int n_terms, float* out, int B,
                  void* ws, size_t ws_bytes, hipStream_t s, bool try_fc) {
  Bufs bf;
  INF_TRY(carve_ws(n, B, 1, ws, ws_bytes, bf));
  if (n_terms == 0) {
    INF_HIP(hipMemsetAsync(out, 0, sizeof(float) * B, s));
    return INF_OK;
  }
  if (try_fc) {
    const int st = fc_series(&n, &x, &vareps, coeff, n_terms, &out, 1, B, s);
    if (st != INF_ERR_UNSUPPORTED) return st;
  }
  const float *xi, *ei;
  INF_TRY(to_internal(n, x, bf.xin, B, s, &xi));
  INF_TRY(to_internal(n, vareps, bf.eps_t, B, s, &ei));
  if (n->fused) return series_fused(&n, &xi, &ei, 1, coeff, n_terms, &out, B, &bf, s);
  INF_TRY(run_forward(n, xi, B, bf, -1, nullptr, s));
  const float* v = ei;
  for (int k = 0; k < n_terms; ++k) {
    float* vo = (k % 2 == 0) ? bf.va : bf.vb;
    INF_TRY(run_vjp(n, v, vo, xi, ei, bf.part + (size_t)k * B * bf.nchunk, B, bf, s));
    v = vo;
  }
  return launch_series_combine(bf.part, coeff, n_terms, B, bf.nchunk, out, s);
}

// neumann_vjp of neumann_logdet_estimator (implicit_block.py:429-436): w = eps + sum_k ncoeff[k] eps^T J^k,
// accumulated in k order into bf.tmp (internal layout).  Leaves the activation derivatives of x saved.
int neumann_w(InfNet* n, const float* xi, const float* ei, const float* ncoeff, int n_terms, int B, Bufs& bf,
              hipStream_t s) {
  const size_t E = (size_t)B * n->d;
  INF_TRY(run_forward(n, xi, B, bf, -1, nullptr, s));
  INF_HIP(hipMemcpyAsync(bf.tmp, ei, sizeof(float) * E, hipMemcpyDeviceToDevice, s));
  const float* v = ei;
  for (int k = 1; k <= n_terms; ++k) {
    float* vo = (k % 2 == 1) ? bf.va : bf.vb;
    INF_TRY(run_vjp(n, v, vo, xi, nullptr, nullptr, B, bf, s));
    INF_TRY(glue_axpy_scaled(bf.tmp, vo, ncoeff[k], (long)E, s));
    v = vo;
  }
  return INF_OK;
}

}  // namespace

// Forward-mode Jacobian of a small fc net: [primal | d tangents] pushed through every layer; returns
// the tangent block (J[i][j] of sample b at t[i*(d+1)*B + (j+1)*B + b]) in *tang.
int inf::fc_jacobian(InfNet* n, const float* x, int B, Bufs& bf, const float** tang, hipStream_t s) {
  const int d = n->d;
  const float* xi;
  INF_TRY(to_internal(n, x, bf.xin, B, s, &xi));
  if (n->fcfused) {
    FcArgs f = fc_args(n, xi, B);
    f.tang = bf.ext1;
    if (fcnet_supported(f, true)) {
      INF_TRY(launch_fcnet(f, true, s));
      *tang = bf.ext1;
      return INF_OK;
    }
  }
  INF_TRY(glue_init_tangents(xi, bf.ext0, d, B, s));
  const int cols = (d + 1) * B;
  const float* cur = bf.ext0;
  for (size_t l = 0; l < n->L.size(); ++l) {
    const WLayer& w = n->L[l];
    float* o = (l % 2 == 0) ? bf.ext1 : bf.ext0;
    GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.A = w.f.A;
    g.M = w.f.M;
    g.Kpad = w.f.Kpad;
    g.Ktot = w.f.K;
    g.X = cur;
    g.x_sample = 0;
    g.P = cols;
    g.N = cols;
    g.H = 1;
    g.W = cols;
    g.out = o;
    g.o_sample = 0;
    g.bias = w.b;
    g.n_primal = B;
    INF_TRY(launch_gemm(g, BL_DIRECT, EP_BIAS_PRIMAL, s));
    if (w.act != ACT_NONE) INF_TRY(launch_fwdmode_act(o, nullptr, w.cout, B, d, w.act, w.act_beta, s));
    cur = o;
  }
  *tang = cur;
  return INF_OK;
}

void inf::logdet_release_thread() {
  int cur = 0;
  (void)hipGetDevice(&cur);
  for (int dev = 0; dev < 16; ++dev) {
    SideStream& ss = g_side[dev];
    if (!ss.s) continue;
    (void)hipSetDevice(dev);
    (void)hipStreamSynchronize(ss.s);
    if (ss.fork) (void)hipEventDestroy(ss.fork);
    if (ss.join) (void)hipEventDestroy(ss.join);
    (void)hipStreamDestroy(ss.s);
    ss = SideStream{};
  }
  (void)hipSetDevice(cur);
}

extern "C" {

// Whole eval pass of an imBlock on fused nets (implicit_block.py:220-234 + 245-322 in eval): the x-net's
// x_embed launch also saves its activation derivatives at x (MODE_EVALSAVE), Broyden solves for z*,
// z = (f_x(x) - f_z(z*)) + x, then the paired power series of both branches with only the z-net's SAVE.
int inf_imblock_eval(InfNet* nx, InfNet* nz, const float* x, float* z, const float* eps_x, const float* eps_z,
                     const float* coeff, int n_terms, float* logdet_x, float* logdet_z, int B, int T, double eps,
                     InfBroydenStats* stats, void* ws, size_t ws_bytes, void* stream) {
  if (!nx || !nz || !x || !z || !eps_x || !eps_z || !coeff || !logdet_x || !logdet_z || B <= 0 || T <= 0 || T > 64 ||
      n_terms < 1 || n_terms > SERIES_MAX || !same_shape(nx, nz))
    return INF_ERR_INVALID;
  if (!fused_pair(nx, nz)) return INF_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const size_t half = ws_need(nx, B, T), zneed = ws_need(nz, B, 1), xneed = ws_need(nx, B, 1);
  if (!ws || ws_bytes < half + zneed) return INF_ERR_WORKSPACE;
  char* w0 = reinterpret_cast<char*>(ws);
  Bufs bfa, bfb, bfc;
  carve(nx, B, T, w0, half, bfa);
  carve(nz, B, 1, w0 + half, zneed, bfb);
  // Overlapped schedule (default; inf_net_set_option(INF_OPT_EVAL_OVERLAP, 0) or INFLOW_EVAL_OVERLAP=0 at create turn it off; needs workspace for a
  // third region): the x-branch series depends only on x, so it runs on a side stream while this stream does the
  // root solve (sync-bound, and short of work at the 8x8 scale) and then the z-branch series; the two streams join
  // before returning.  Concurrent series launches also desynchronise the CUs' d1/d2 bursts (every 1-WG/CU tile
  // of one launch reads its derivatives in the same phase): 2268 -> 2432 samples/s at B=64 with the 128-pixel VJP.
  // The series terms run on the 128-pixel VJP kernel only where a launch's grid covers every CU (net313_family), and
  // single-net launches that each hold a whole CU per workgroup alternate rather than share the GPU.  So where the
  // pair launch reaches that kernel and a single-net launch would be demoted to the 64-pixel one, the block takes the
  // sequential pair schedule: one pair launch per term beats two demoted launches, by more than the overlap hides
  // of the root solve.
  const bool demoted = series_family(nx, nz, B, 2) == FAM_K128 &&
                       (series_family(nx, nx, B, 1) != FAM_K128 || series_family(nz, nz, B, 1) != FAM_K128);
  const bool overlap = nx->eval_overlap && !demoted && ws_bytes >= half + zneed + xneed;
  if (overlap) {
    carve(nx, B, 1, w0 + half + zneed, xneed, bfc);
    bfc.D = bfa.D;                              // the x_embed pass saves f_x's derivatives into bfa.D
  }
  const int layout = overlap ? 1 : 2;           // single-net series launches, or the pair's tile layout
  // x_embed = f_x(x) + x, saving f_x's derivatives at x (implicit_block.py:71)
  {
    Net313Args f = net313_args(nx, x, B, bfa, false);
    INF_TRY(launch_net313_multi(&f, 1, nx->fhid, MODE_EVALSAVE, s, layout));
    OutArgs a;
    memset(&a, 0, sizeof(a));
    a.bias = nx->L[2].b;
    a.in0 = x;
    a.out0 = bfa.fx;
    a.out1 = bfa.xemb;
    INF_TRY(out_stage(nx, fused_taps(nx), OM_EMBED, a, bfa.Y, B, s));
  }
  SideJoin join;
  if (overlap) {
    SideStream* side = side_stream();
    if (!side) return INF_ERR_HIP;
    INF_HIP(hipEventRecord(side->fork, s));
    INF_HIP(hipStreamWaitEvent(side->s, side->fork, 0));
    join.side = side;
    join.s = s;
    INF_TRY(series_fused(&nx, &x, &eps_x, 1, coeff, n_terms, &logdet_x, B, &bfc, side->s, /*save_mask=*/0u, nullptr, nullptr,
                         /*concurrent=*/2));
  }
  InfBroydenStats st = stats_for(stats);
  INF_TRY(broyden_solve(nz, x, B, T, eps, &st, nullptr, bfa, s));
  if (stats) *stats = st;
  if (!st.prot_break) {
    INF_TRY(glue_recomp(bfa.fx, bfa.flow, x, z, (long)B * nx->d, s));
  } else {
    OutArgs a;
    memset(&a, 0, sizeof(a));
    a.in0 = bfa.fx;
    a.in1 = x;
    a.out0 = z;
    INF_TRY(run_forward(nz, bfa.lowest, B, bfa, OM_RECOMP, &a, s));
  }
  if (overlap) {
    const float* zin = z;
    return series_fused(&nz, &zin, &eps_z, 1, coeff, n_terms, &logdet_z, B, &bfb, s, /*save_mask=*/1u, nullptr, nullptr,
                        /*concurrent=*/2);   // join: ~SideJoin
  }
  InfNet* nets[2] = {nx, nz};
  const float* xs[2] = {x, z};
  const float* es[2] = {eps_x, eps_z};
  float* outs[2] = {logdet_x, logdet_z};
  Bufs bfs[2] = {bfa, bfb};
  return series_fused(nets, xs, es, 2, coeff, n_terms, outs, B, bfs, s, /*save_mask=*/2u);
}

int inf_imblock_eval_exact(InfNet* nx, InfNet* nz, const float* x, float* z, float* logdet_x, float* logdet_z, int B,
                           int T, double eps, InfBroydenStats* stats, void* ws, size_t ws_bytes, void* stream) {
  if (!nx || !nz || !x || !z || !logdet_x || !logdet_z || B <= 0 || T <= 0 || T > 64 || !same_shape(nx, nz))
    return INF_ERR_INVALID;
  INF_TRY(eval_exact_check(nx, nz, x, B));
  Bufs bf;
  INF_TRY(carve_ws(nz, B, T, ws, ws_bytes, bf));
  return eval_exact_fc(nx, nz, x, z, logdet_x, logdet_z, B, T, eps, stats, bf, (hipStream_t)stream, false, nullptr);
}

size_t inf_flow_chain_workspace_bytes(InfNet* const* net_z, int n_blocks, int batch, const int* thresholds) {
  if (!net_z || n_blocks <= 0 || batch <= 0 || !thresholds) return 0;
  size_t blk = 0;
  for (int i = 0; i < n_blocks; ++i)
    if (net_z[i]) blk = std::max(blk, inf_workspace_bytes(net_z[i], batch, thresholds[i]));
  const size_t d = net_z[0] ? (size_t)net_z[0]->d : 0;
  // two block workspaces (consecutive blocks alternate: the pair launch writes the next block's buffers while this
  // block's are live), two z and logp buffers, two logdet_x / logdet_z pairs
  return 2 * ((blk + 255) & ~(size_t)255) + 256 * 8 + sizeof(float) * ((size_t)2 * batch * d + (size_t)6 * batch);
}

// SequentialFlow of fc imBlocks in eval (train_tabular.py:314-336; container.py:12-20): block i is
// inf_imblock_eval_exact on the previous block's z, its log-density step logp <- logp - (logdet_x - logdet_z) on the device
// (implicit_block.py:234), the blocks back to back on the stream with no host round trip between them beyond the ones a
// block itself makes.  On the launch path (global rule, f16x3 nets) block i's z-branch Jacobian launch also evaluates
// block i + 1's x-branch (FcNextX): consecutive blocks alternate between two workspaces and logdet buffers.
int inf_flow_eval_exact_chain(InfNet* const* net_x, InfNet* const* net_z, int n_blocks, const float* x, float* z,
                              const float* logp_in, float* logp_out, int B, const int* thresholds, const double* eps,
                              InfBroydenStats* stats, void* ws, size_t ws_bytes, void* stream) {
  // logp_in == logp_out is refused: a block's log-density step is folded into its z-branch launch, which runs again
  // when the predicted last iterate was not the result, and would then read the already-updated log p
  if (!net_x || !net_z || n_blocks <= 0 || !x || !z || !logp_out || B <= 0 || !thresholds || !eps || x == z ||
      logp_in == logp_out)
    return INF_ERR_INVALID;
  for (int i = 0; i < n_blocks; ++i) {
    InfNet *nx = net_x[i], *nz = net_z[i];
    if (!nx || !nz || !same_shape(nx, nz) || !same_shape(nz, net_z[0]) || thresholds[i] <= 0 || thresholds[i] > 64)
      return INF_ERR_INVALID;
    INF_TRY(eval_exact_check(nx, nz, x, B));
  }
  if (!ws || ws_bytes < inf_flow_chain_workspace_bytes(net_z, n_blocks, B, thresholds)) return INF_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const size_t E = (size_t)B * net_z[0]->d;
  size_t blk = 0;
  for (int i = 0; i < n_blocks; ++i) blk = std::max(blk, inf_workspace_bytes(net_z[i], B, thresholds[i]));
  blk = (blk + 255) & ~(size_t)255;
  char* base = reinterpret_cast<char*>(ws);
  size_t off = 2 * blk;
  auto take = [&](size_t bytes) {
    off = (off + 255) & ~(size_t)255;
    char* p = base + off;
    off += bytes;
    return reinterpret_cast<float*>(p);
  };
  float* zb[2] = {take(sizeof(float) * E), take(sizeof(float) * E)};
  float* ldx[2] = {take(sizeof(float) * B), take(sizeof(float) * B)};
  float* ldz[2] = {take(sizeof(float) * B), take(sizeof(float) * B)};
  float* lp[2] = {take(sizeof(float) * B), take(sizeof(float) * B)};
  Bufs bfs[2];
  auto carve_block = [&](int i) {
    return carve_ws(net_z[i], B, thresholds[i], base + (size_t)(i & 1) * blk, blk, bfs[i & 1]);
  };
  INF_TRY(carve_block(0));
  const float* in = x;
  const float* lin = logp_in;
  bool x_done = false;
  for (int i = 0; i < n_blocks; ++i) {
    const bool last = i == n_blocks - 1;
    float* out = last ? z : zb[i & 1];
    float* lout = last ? logp_out : lp[i & 1];
    FcNextX nxt;
    FcNextX* np = nullptr;
    if (!last) {
      INF_TRY(carve_block(i + 1));
      if (!fc_block_first(net_z[i]) && !fc_block_first(net_z[i + 1]) && fc_pair_ok(net_z[i], net_x[i + 1])) {
        nxt.nx = net_x[i + 1];
        nxt.bf = &bfs[(i + 1) & 1];
        nxt.logdet = ldx[(i + 1) & 1];
        np = &nxt;
      }
    }
    FcLogpStep lps;
    lps.lin = lin;
    lps.lout = lout;
    INF_TRY(eval_exact_fc(net_x[i], net_z[i], in, out, ldx[i & 1], ldz[i & 1], B, thresholds[i], eps[i],
                          stats ? &stats[i] : nullptr, bfs[i & 1], s, x_done, np, &lps));
    if (!lps.done) INF_TRY(glue_logp_step(lin, ldx[i & 1], ldz[i & 1], lout, B, s));
    x_done = np && nxt.done;
    in = out;
    lin = lout;
  }
  return INF_OK;
}

int inf_logdet_series(InfNet* n, const float* x, const float* vareps, const float* coeff, int n_terms, float* out,
                      int B, void* ws, size_t ws_bytes, void* stream) {
  if (!n || !x || !vareps || !coeff || !out || B <= 0 || n_terms < 0 || n_terms > SERIES_MAX) return INF_ERR_INVALID;
  return series_single(n, x, vareps, coeff, n_terms, out, B, ws, ws_bytes, (hipStream_t)stream, true);
}

// Both log-det series of an imBlock (x-branch and z-branch, implicit_block.py:318-322) advanced in
// lockstep: when both nets take the fused path, every term is ONE launch over both nets' tiles.
// ws must hold 2 x inf_workspace_bytes(net, batch, 1).
int inf_logdet_series_pair(InfNet* na, const float* xa, const float* ea, InfNet* nb, const float* xb, const float* eb,
                           const float* coeff, int n_terms, float* out_a, float* out_b, int B, void* ws,
                           size_t ws_bytes, void* stream) {
  if (!na || !nb || !xa || !xb || !ea || !eb || !coeff || !out_a || !out_b || B <= 0 || n_terms < 0 ||
      n_terms > SERIES_MAX || !same_shape(na, nb))
    return INF_ERR_INVALID;
  const size_t half = ws_need(na, B, 1);
  if (!ws || ws_bytes < 2 * half) return INF_ERR_WORKSPACE;
  char* w0 = reinterpret_cast<char*>(ws);
  hipStream_t s = (hipStream_t)stream;
  InfNet* nets[2] = {na, nb};
  const float* xs[2] = {xa, xb};
  const float* es[2] = {ea, eb};
  float* outs[2] = {out_a, out_b};
  if (n_terms > 0) {
    const int st = fc_series(nets, xs, es, coeff, n_terms, outs, 2, B, s);
    if (st != INF_ERR_UNSUPPORTED) return st;
  }
  if (!fused_pair(na, nb)) {
    INF_TRY(series_single(na, xa, ea, coeff, n_terms, out_a, B, w0, half, s, false));
    return series_single(nb, xb, eb, coeff, n_terms, out_b, B, w0 + half, half, s, false);
  }
  Bufs bfs[2];
  carve(na, B, 1, w0, half, bfs[0]);
  carve(nb, B, 1, w0 + half, half, bfs[1]);
  if (n_terms == 0) {
    INF_HIP(hipMemsetAsync(out_a, 0, sizeof(float) * B, s));
    INF_HIP(hipMemsetAsync(out_b, 0, sizeof(float) * B, s));
    return INF_OK;
  }
  return series_fused(nets, xs, es, 2, coeff, n_terms, outs, B, bfs, s);
}

int inf_neumann_vector(InfNet* n, const float* x, const float* vareps, const float* ncoeff, int n_terms, float* w,
                       int B, void* ws, size_t ws_bytes, void* stream) {
  if (!n || !x || !vareps || !ncoeff || !w || B <= 0 || n_terms < 0) return INF_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  Bufs bf;
  INF_TRY(carve_ws(n, B, 1, ws, ws_bytes, bf));
  const float *xi, *ei;
  INF_TRY(to_internal(n, x, bf.xin, B, s, &xi));
  INF_TRY(to_internal(n, vareps, bf.eps_t, B, s, &ei));
  INF_TRY(neumann_w(n, xi, ei, ncoeff, n_terms, B, bf, s));
  return to_boundary(n, bf.tmp, w, B, s);
}

// Both nets' Neumann vectors (x- and z-branch of an imBlock's training log-det) in lockstep: one fused VJP
// launch per term for both nets with the accumulation folded into the next term's staging.  Nets off the
// fused path (or n_terms == 0) fall back to two inf_neumann_vector computations.
int inf_neumann_vector_pair(InfNet* na, const float* xa, const float* ea, InfNet* nb, const float* xb,
                            const float* eb, const float* ncoeff, int n_terms, float* wa, float* wb, int B, void* ws,
                            size_t ws_bytes, void* stream) {
  if (!na || !nb || !xa || !xb || !ea || !eb || !ncoeff || !wa || !wb || B <= 0 || n_terms < 0 || !same_shape(na, nb))
    return INF_ERR_INVALID;
  const size_t half = ws_bytes / 2;
  char* w1 = reinterpret_cast<char*>(ws) + half;
  if (!fused_pair(na, nb) || n_terms == 0) {
    INF_TRY(inf_neumann_vector(na, xa, ea, ncoeff, n_terms, wa, B, ws, half, stream));
    return inf_neumann_vector(nb, xb, eb, ncoeff, n_terms, wb, B, w1, half, stream);
  }
  hipStream_t s = (hipStream_t)stream;
  Bufs bfs[2];
  INF_TRY(carve_ws(na, B, 1, ws, half, bfs[0]));
  INF_TRY(carve_ws(nb, B, 1, w1, half, bfs[1]));
  InfNet* nets[2] = {na, nb};
  const float* xs[2] = {xa, xb};
  const float* es[2] = {ea, eb};
  float* wouts[2] = {wa, wb};
  float* outs[2] = {nullptr, nullptr};
  return series_fused(nets, xs, es, 2, nullptr, n_terms, outs, B, bfs, s, 3u, wouts, ncoeff);
}

int inf_logdet_neumann(InfNet* n, const float* x, const float* vareps, const float* ncoeff, int n_terms, float* out,
                       int B, void* ws, size_t ws_bytes, void* stream) {
  if (!n || !x || !vareps || !ncoeff || !out || B <= 0 || n_terms < 0) return INF_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  Bufs bf;
  INF_TRY(carve_ws(n, B, 1, ws, ws_bytes, bf));
  const float *xi, *ei;
  INF_TRY(to_internal(n, x, bf.xin, B, s, &xi));
  INF_TRY(to_internal(n, vareps, bf.eps_t, B, s, &ei));
  INF_TRY(neumann_w(n, xi, ei, ncoeff, n_terms, B, bf, s));
  INF_TRY(run_vjp(n, bf.tmp, bf.va, xi, ei, bf.part, B, bf, s));
  const float one = 1.f;
  return launch_series_combine(bf.part, &one, 1, B, bf.nchunk, out, s);
}

int inf_logdet_exact(InfNet* n, const float* x, float* out, int B, void* ws, size_t ws_bytes, void* stream) {
  if (!n || !x || !out || B <= 0) return INF_ERR_INVALID;
  if (!n->fc || n->d > 16 || n->pre_act != ACT_NONE) return INF_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  Bufs bf;
  INF_TRY(carve_ws(n, B, 1, ws, ws_bytes, bf));
  if (n->fcfused) {                   // forward-mode Jacobian and the LU in one launch
    const float* xi;
    INF_TRY(to_internal(n, x, bf.xin, B, s, &xi));
    FcArgs f = fc_args(n, xi, B);
    f.logdet = out;
    if (fcnet_supported(f, true)) return launch_fcnet(f, true, s);
  }
  const float* tang = nullptr;
  INF_TRY(fc_jacobian(n, x, B, bf, &tang, s));
  return launch_logdet_small(tang, out, n->d, B, B, s);
}

int inf_logdet_exact_trace(InfNet* n, const float* x, const float* coeff, int n_terms, float* out, int B, void* ws,
                           size_t ws_bytes, void* stream) {
  if (!n || !x || !coeff || !out || B <= 0 || n_terms < 1 || n_terms > SERIES_MAX) return INF_ERR_INVALID;
  if (!n->fc || n->d > 16 || n->pre_act != ACT_NONE) return INF_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  Bufs bf;
  INF_TRY(carve_ws(n, B, 1, ws, ws_bytes, bf));
  const float* tang = nullptr;
  INF_TRY(fc_jacobian(n, x, B, bf, &tang, s));
  return launch_trace_series(tang, coeff, n_terms, out, n->d, B, B, s);
}

}  // extern "C"
