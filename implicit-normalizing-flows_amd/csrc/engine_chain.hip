// The launch chains of one net evaluation: the forward pass (per-layer GEMMs, the fused 3-1-3 launch or the fused fc
// launch) with its output stage, the VJP, and the boundary-layout transposes of fc nets.
//
// Reference mapping (implicit_block.py):
//   inf_net_forward       <- nnet(x)                      (nn.Sequential of InducedNorm + Swish/Sin)
//   inf_net_vjp           <- torch.autograd.grad(g, x, v)                                   (:422)
#include "engine.h"

using namespace inf;

// ---------------------------------------------------------------------------------------------
// GEMM argument builders
// ---------------------------------------------------------------------------------------------
GemmArgs inf::gemm_base(const InfNet* n, const Operand& op, const float* X, int in_ch, int B) {
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.x6 = n->mfma_mode != INF_MFMA_F32;
  g.A = op.A;
  g.M = op.M;
  g.Kpad = op.Kpad;
  g.Ktot = op.K;
  g.X = X;
  if (n->fc) {        // feature-major (ch, B): one "image" with B pixels
    g.P = B;
    g.N = B;
    g.x_sample = 0;
    g.H = 1;
    g.W = B;
  } else {
    g.P = n->P;
    g.N = B * n->P;
    g.x_sample = (long)in_ch * n->P;
    g.H = n->H;
    g.W = n->W;
  }
  return g;
}

void inf::set_out(const InfNet* n, GemmArgs& g, float* out, int out_rows) {
  g.out = out;
  g.o_sample = n->fc ? 0 : (long)out_rows * n->P;
}

// Every per-layer GEMM of the unfused chains (forward, VJP, gradient chain).  The layers of an fc net over more than
// FC_NARROW_MAX features take the skinny family (gemm_skinny.hip: (d, B) tensors have N = B columns, which leaves
// launch_gemm's 128 x 128 tile 1 - 24 workgroups) unless INF_OPT_FC_SKINNY is 0 or N alone gives the 128 x 128 tiling a
// workgroup per CU (256); everything else -- conv nets, narrow fc nets -- calls launch_gemm exactly as before.
int inf::layer_gemm(const InfNet* n, const GemmArgs& g, int load, int epi, float* kslab, size_t kslab_bytes,
                    hipStream_t s) {
  if (n->fc && n->d > FC_NARROW_MAX && n->fc_skinny && load == BL_DIRECT && epi != EP_BIAS_PRIMAL &&
      (long)((g.M + 127) / 128) * ((g.N + 127) / 128) < 256)
    return launch_gemm_skinny(g, epi, kslab, kslab_bytes, s);
  return launch_gemm(g, load, epi, s);
}

Net313Args inf::net313_args(const InfNet* n, const float* in, int B, Bufs& bf, bool vjp) {
  Net313Args f;
  memset(&f, 0, sizeof(f));
  f.in = in;
  f.pre_beta = vjp ? nullptr : n->pre_beta;
  // another fused activation than Swish (Sin / ELU / Softplus / ReLU; the eligibility check made all of the net's the same)
  f.act = n->L[0].act == ACT_SWISH ? 0 : n->L[0].act;
  f.pre_act = (vjp || n->pre_act == ACT_SWISH) ? 0 : n->pre_act;
  f.A1 = vjp ? n->F1b : n->F1f;
  f.K1pad = n->K1pad;
  f.A2 = vjp ? n->F2b : n->F2f;
  f.A3 = vjp ? n->F3b : n->F3f;
  const bool spl = n->mfma_mode != INF_MFMA_F32;
  const bool h3 = n->mfma_mode == INF_MFMA_F16X3;
  f.A1s = spl ? (const void*)n->Fs[vjp ? 1 : 0] : nullptr;
  f.A2s = spl ? (const void*)n->Fs[vjp ? 3 : 2] : nullptr;
  f.A3s = spl ? (const void*)n->Fs[vjp ? 5 : 4] : nullptr;
  f.A1h = h3 ? (const void*)n->Fh[vjp ? 1 : 0] : nullptr;
  f.A2h = h3 ? (const void*)n->Fh[vjp ? 3 : 2] : nullptr;
  f.A3h = h3 ? (const void*)n->Fh[vjp ? 5 : 4] : nullptr;
  f.Ah_exp = h3 ? n->Fexp + (vjp ? 3 : 0) : nullptr;
  f.A3p = h3 ? (const void*)n->Fhp[vjp ? 1 : 0] : nullptr;
  f.M3 = n->M3;
  f.M3pad = n->M3pad;
  f.b1 = n->L[0].b;
  f.beta1 = n->L[0].act_beta;
  f.b2 = n->L[1].b;
  f.beta2 = n->L[1].act_beta;
  f.d1 = bf.D[0];
  f.d2 = bf.D[1];
  f.Y = bf.Y;
  f.B = B;
  f.C = n->C;
  f.H = n->H;
  f.W = n->W;
  f.seg = n->W < 64 ? n->W : 64;
  f.k128 = n->k128;
  f.exact_scale = n->exact_scale;
  f.presplit = n->presplit;
  return f;
}

FcArgs inf::fc_args(const InfNet* n, const float* x, int B) {
  FcArgs f;
  memset(&f, 0, sizeof(f));
  f.nl = (int)n->L.size();
  f.d = n->d;
  f.B = B;
  f.act = n->L[0].act;
  const bool h3 = n->mfma_mode == INF_MFMA_F16X3 && n->fch;
  f.tan_fixed = 1;
  for (const WLayer& w : n->L) f.tan_fixed &= w.coeff <= 1.f;
  for (int l = 0; l < f.nl && l < FC_MAXL; ++l) {
    f.L[l].A = n->L[l].f.A;
    f.L[l].Ah = h3 ? n->fch + n->fch_off[l] : nullptr;
    f.L[l].Aexp = h3 ? n->fchexp + l : nullptr;
    f.L[l].Kpad = n->L[l].f.Kpad;
    f.L[l].b = n->L[l].b;
    f.L[l].beta = n->L[l].act_beta;
  }
  f.x = x;
  return f;
}

int inf::out_stage(const InfNet* n, const Operand& op, int mode, OutArgs a, float* Y, int B, hipStream_t s) {
  a.Y = Y;
  a.y_sample = n->fc ? 0 : (long)op.M * n->P;
  a.C = n->C;
  a.H = n->H;
  a.W = n->W;
  a.ks = op.taps ? 3 : 1;
  a.mode = mode;
  return n->fc ? launch_fc_out(a, B, s) : launch_conv_out(a, B, s);
}

// Forward chain.  mode = OM_* for the output stage, or -1 for "save derivatives only" (log-det prep:
// the last layer is skipped, D[l] = act'(a_l) are kept).  x is in internal layout.
int inf::run_forward(InfNet* n, const float* x, int B, Bufs& bf, int mode, const OutArgs* oa, hipStream_t s) {
  const int L = (int)n->L.size();
  if (n->fcfused && mode >= OM_PLAIN && mode <= OM_RECOMP) {   // the whole net and fc_out's epilogue in one launch
    FcArgs f = fc_args(n, x, B);
    f.o = *oa;
    f.o.mode = mode;
    f.o.bias = n->L[L - 1].b;
    return launch_fcnet(f, false, s);
  }
  if (n->fused) {
    Net313Args f = net313_args(n, x, B, bf, false);
    INF_TRY(launch_net313(f, n->fhid, mode < 0 ? MODE_SAVE : MODE_EVAL, s));
    if (mode < 0) return INF_OK;
    OutArgs a = *oa;
    a.bias = n->L[2].b;
    a.pre_beta = nullptr;
    return out_stage(n, fused_taps(n), mode, a, bf.Y, B, s);
  }
  const float* cur = x;
  int cur_ch = n->C;
  for (int l = 0; l < L - 1; ++l) {
    const WLayer& w = n->L[l];
    float* out = (l % 2 == 0) ? bf.h0 : bf.h1;
    GemmArgs g = gemm_base(n, w.f, cur, cur_ch, B);
    g.pre_beta = (l == 0) ? n->pre_beta : nullptr;
    g.pre_act = (l == 0) ? n->pre_act : ACT_NONE;
    set_out(n, g, out, w.cout);
    g.bias = w.b;
    g.act = w.act;
    g.act_beta = w.act_beta;
    g.deriv_out = (mode < 0) ? bf.D[l] : nullptr;
    g.write_out = (mode < 0 && l == L - 2) ? 0 : 1;
    INF_TRY(layer_gemm(n, g, w.f.load, EP_BIAS_ACT, bf.kslab, bf.kslab_bytes, s));
    cur = out;
    cur_ch = w.cout;
  }
  if (mode < 0) return INF_OK;
  const WLayer& w = n->L[L - 1];
  GemmArgs g = gemm_base(n, w.f, cur, cur_ch, B);
  g.pre_beta = (L == 1) ? n->pre_beta : nullptr;
  g.pre_act = (L == 1) ? n->pre_act : ACT_NONE;
  set_out(n, g, bf.Y, w.f.M);
  INF_TRY(layer_gemm(n, g, w.f.load, EP_STORE, bf.kslab, bf.kslab_bytes, s));
  OutArgs a = *oa;
  a.bias = w.b;
  a.pre_beta = nullptr;
  return out_stage(n, w.f, mode, a, bf.Y, B, s);
}

// One VJP: vout = v^T J(x), using D saved by run_forward(mode=-1) on x.  partial (B x nchunk doubles,
// may be null) receives the per-sample partial sums of vout . eps.
int inf::run_vjp(InfNet* n, const float* v, float* vout, const float* xin, const float* eps, double* partial, int B,
                 Bufs& bf, hipStream_t s) {
  const int L = (int)n->L.size();
  OutArgs a;
  memset(&a, 0, sizeof(a));
  a.in0 = eps;
  a.in1 = xin;
  a.out0 = vout;
  a.pre_beta = n->pre_beta;
  a.pre_act = n->pre_act;
  a.partial = partial;
  a.nchunk = n->fc ? fc_nchunk(n->d) : out_nchunk(n->d);
  if (n->fused) {
    Net313Args f = net313_args(n, v, B, bf, true);
    INF_TRY(launch_net313(f, n->fhid, MODE_VJP, s));
    return out_stage(n, fused_taps(n), OM_VJP, a, bf.Y, B, s);
  }
  const float* cur = v;
  int cur_ch = n->C;
  for (int l = L - 1; l >= 1; --l) {
    const WLayer& w = n->L[l];
    float* out = ((L - 1 - l) % 2 == 0) ? bf.h0 : bf.h1;
    GemmArgs g = gemm_base(n, w.g, cur, cur_ch, B);
    set_out(n, g, out, w.cin);
    g.deriv_in = bf.D[l - 1];
    INF_TRY(layer_gemm(n, g, w.g.load, EP_MUL_DERIV, bf.kslab, bf.kslab_bytes, s));
    cur = out;
    cur_ch = w.cin;
  }
  const WLayer& w = n->L[0];
  GemmArgs g = gemm_base(n, w.g, cur, cur_ch, B);
  set_out(n, g, bf.Y, w.g.M);
  INF_TRY(layer_gemm(n, g, w.g.load, EP_STORE, bf.kslab, bf.kslab_bytes, s));
  return out_stage(n, w.g, OM_VJP, a, bf.Y, B, s);
}

int inf::to_internal(InfNet* n, const float* x, float* buf, int B, hipStream_t s, const float** xi) {
  *xi = n->fc ? buf : x;
  return n->fc ? launch_transpose(x, buf, B, n->d, s) : INF_OK;
}
int inf::to_boundary(InfNet* n, const float* xi, float* out, int B, hipStream_t s) {
  if (!n->fc) {
    if (xi != out) INF_HIP(hipMemcpyAsync(out, xi, sizeof(float) * (size_t)B * n->d, hipMemcpyDeviceToDevice, s));
    return INF_OK;
  }
  return launch_transpose(xi, out, n->d, B, s);
}

extern "C" {

int inf_net_forward(InfNet* n, const float* x, float* y, int B, void* ws, size_t ws_bytes, void* stream) {
  if (!n || !x || !y || B <= 0) return INF_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  Bufs bf;
  INF_TRY(carve_ws(n, B, 1, ws, ws_bytes, bf));
  const float* xi;
  INF_TRY(to_internal(n, x, bf.xin, B, s, &xi));
  OutArgs a;
  memset(&a, 0, sizeof(a));
  return write_boundary(n, bf, y, B, s, [&](float* o) {
    a.out0 = o;
    return run_forward(n, xi, B, bf, OM_PLAIN, &a, s);
  });
}

int inf_net_vjp(InfNet* n, const float* x, const float* v, float* out, int B, void* ws, size_t ws_bytes,
                void* stream) {
  if (!n || !x || !v || !out || B <= 0) return INF_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  Bufs bf;
  INF_TRY(carve_ws(n, B, 1, ws, ws_bytes, bf));
  const float *xi, *vi;
  INF_TRY(to_internal(n, x, bf.xin, B, s, &xi));
  INF_TRY(to_internal(n, v, bf.eps_t, B, s, &vi));
  INF_TRY(run_forward(n, xi, B, bf, -1, nullptr, s));
  return write_boundary(n, bf, out, B, s,
                        [&](float* o) { return run_vjp(n, vi, o, xi, nullptr, nullptr, B, bf, s); });
}

}  // extern "C"
