// Parameter gradients (training path) on the generic GEMM operands (W_eff packed at refresh).
// Nets whose intermediate activations are Swish or Sin: layer l computes h_l = W_l * in_l + b_l,
// in_0 = preact(x), in_l = act(h_{l-1}) (applied once from the stored pre-activation).  Conv nets in their (B, C, H, W)
// layout; fc nets feature-major (d, N), N columns as one image of N pixels (gemm_base) -- the C-ABI entries transpose
// the (B, d) boundary tensors in and out.
//
// Reference mapping (implicit_block.py):
//   inf_net_param_grad      <- the recompute graph of the training forward                (:226-227)
//   inf_net_surrogate_grad  <- the memory-efficient Neumann estimator's surrogate         (:388-394, 437-438)
//   inf_logdet_grad         <- autograd through the fc log-det estimators (train_tabular.py / train_toy.py)
#include "engine.h"

using namespace inf;

namespace {

constexpr int GRAD_SPLIT = 32;
constexpr int GRAD_BLOCKS = 512;

size_t carve_grad(const InfNet* n, int B, void* ws, size_t cap, GradBufs& g) {
  WS w{reinterpret_cast<char*>(ws), cap, 0};
  const size_t hid = (size_t)B * n->hidden_max * n->P, in = (size_t)B * n->d;
  const int L = (int)n->L.size();
  size_t mn = 1;
  for (const auto& l : n->L) mn = std::max(mn, (size_t)l.cout * l.cin * l.ks * l.ks);
  g.H.resize(L > 0 ? L - 1 : 0);
  g.Hd.resize(L > 0 ? L - 1 : 0);
  g.Ad.resize(L > 0 ? L : 0);
  for (auto& p : g.H) p = w.take<float>(hid);
  for (auto& p : g.Hd) p = w.take<float>(hid);
  for (int l = 0; l < L; ++l) g.Ad[l] = w.take<float>(l == 0 ? in : hid);
  g.A.resize(L > 0 ? L : 0);
  for (int l = 0; l < L; ++l) g.A[l] = w.take<float>(l == 0 ? in : hid);
  for (float** p : {&g.gA, &g.gB, &g.hA, &g.hB, &g.gad, &g.ga}) *p = w.take<float>(std::max(hid, in));
  g.Y = w.take<float>((size_t)B * n->rows_max * n->P);
  g.slab = w.take<float>((size_t)GRAD_SPLIT * mn);
  g.dWe = w.take<float>(mn);
  g.dWe2 = w.take<float>(mn);
  g.dsig = w.take<float>(mn);
  g.xin = w.take<float>(in);
  g.tmp_in = w.take<float>(in);
  for (float** p : {&g.x_t, &g.w_t, &g.e_t, &g.gx_t}) *p = n->fc ? w.take<float>(in) : nullptr;
  g.act = w.take<float>(std::max(hid, in));   // swish of a stored pre-activation (weight-gradient operand)
  g.bpart = w.take<double>(std::max<size_t>(GRAD_BLOCKS + 64, glue_batched_dot_scratch(B, (long)n->hidden_max * n->P) + 64));
  g.dot = w.take<double>(128);      // [0] the dot, [1..64] its block partials
  g.max_split = GRAD_SPLIT;
  g.kslab_bytes = (n->fc && n->d > FC_NARROW_MAX) ? SKINNY_SLAB_BYTES : 0;
  g.kslab = g.kslab_bytes ? w.take<float>(g.kslab_bytes / sizeof(float)) : nullptr;
  return w.off + 256;
}

// Input of layer l as the GEMMs consume it: x (l = 0) or H[l-1], with its swish (preact / activation)
// applied once into gb.A[l] instead of in every output tile's loader.  Returns the operand, no beta left.
int layer_input(InfNet* n, int l, const float* x, GradBufs& gb, int B, hipStream_t s, const float** out) {
  const float* in = l == 0 ? x : gb.H[l - 1];
  const int act = l == 0 ? n->pre_act : n->L[l - 1].act;
  const float* pb = l == 0 ? n->pre_beta : n->L[l - 1].act_beta;
  if (act == ACT_NONE) {
    *out = in;
    return INF_OK;
  }
  const long ne = (long)B * n->L[l].cin * n->P;
  INF_TRY(launch_act_apply(in, act, pb, gb.A[l], ne, s));
  *out = gb.A[l];
  return INF_OK;
}

// h_l = W_l * in (+ b_l); in gets swish(., pre_beta) on load when pre_beta is set.  l < L-1 (no taps).
int layer_fwd(InfNet* n, int l, const float* in, const float* pre_beta, bool bias, float* out, int B, GradBufs& gb,
              hipStream_t s) {
  const WLayer& w = n->L[l];
  GemmArgs g = gemm_base(n, w.f, in, w.cin, B);
  g.pre_beta = pre_beta;
  set_out(n, g, out, w.cout);
  g.bias = bias ? w.b : nullptr;
  return layer_gemm(n, g, w.f.load, bias ? EP_BIAS : EP_STORE, gb.kslab, gb.kslab_bytes, s);
}

// out = W_l^T gout  (input-side gradient of layer l, no activation factor)
int layer_vjp(InfNet* n, int l, const float* gout, float* out, int B, GradBufs& gb, hipStream_t s) {
  const WLayer& w = n->L[l];
  GemmArgs g = gemm_base(n, w.g, gout, w.cout, B);
  if (w.g.taps) {                       // (the first layer of a conv net: w.cin == n->C)
    set_out(n, g, gb.Y, w.g.M);
    INF_TRY(launch_gemm(g, w.g.load, EP_STORE, s));
    OutArgs a;
    memset(&a, 0, sizeof(a));
    a.out0 = out;
    return out_stage(n, w.g, OM_VJP, a, gb.Y, B, s);
  }
  set_out(n, g, out, w.cin);
  return layer_gemm(n, g, w.g.load, EP_STORE, gb.kslab, gb.kslab_bytes, s);
}

// dW_eff of layer l = sum_{b,p} G (x) X~ (accumulate: add into gb.dWe), X = in_l
int layer_wgrad(InfNet* n, int l, const float* G, const float* X, const float* x_beta, float* out, int B, GradBufs& gb,
                hipStream_t s) {
  const WLayer& w = n->L[l];
  WgradArgs a;
  memset(&a, 0, sizeof(a));
  a.G = G;
  a.X = X;
  a.x_beta = x_beta;
  a.B = n->fc ? 1 : B;               // fc: one image of B columns
  a.P = n->fc ? B : n->P;
  a.H = n->fc ? 1 : n->H;
  a.W = n->fc ? B : n->W;
  a.g_sample = (long)w.cout * a.P;
  a.x_sample = (long)w.cin * a.P;
  a.ks = w.ks;
  a.M = w.cout;
  a.N = w.cin * w.ks * w.ks;
  a.slab = gb.slab;
  a.out = out;
  a.max_split = gb.max_split;
  a.fc = n->fc ? 1 : 0;              // (rows, columns) matrices: grad.hip wgrad_fc_kernel
  return launch_wgrad(a, s);
}

// dW (raw weight) from dW_eff through W_eff = W / max(1, sigma / coeff), sigma = u . (W v)
int layer_sigma_chain(InfNet* n, int l, const float* dWe, float* dW, GradBufs& gb, hipStream_t s) {
  const WLayer& w = n->L[l];
  const bool spatial = w.ks > 1;
  WgradArgs a;                                  // dsigma/dW = u (x) v~ (one "sample")
  memset(&a, 0, sizeof(a));
  a.G = w.u;
  a.X = w.v;
  a.B = 1;
  a.P = spatial ? n->P : 1;
  a.H = spatial ? n->H : 1;
  a.W = spatial ? n->W : 1;
  a.g_sample = (long)w.cout * a.P;
  a.x_sample = (long)w.cin * a.P;
  a.ks = w.ks;
  a.M = w.cout;
  a.N = w.cin * w.ks * w.ks;
  a.slab = gb.slab;
  a.out = gb.dsig;
  a.max_split = gb.max_split;
  INF_TRY(launch_wgrad(a, s));
  return launch_sigma_chain(dWe, w.W, gb.dsig, w.factor, w.coeff, gb.dot, dW, (long)w.cout * w.cin * w.ks * w.ks, s);
}

bool grad_supported(const InfNet* n) {
  if (n->L.empty()) return false;
  // Swish / Sin only: the parameter-gradient kernels carry these two's second derivatives (grad.hip); a bias-free
  // layer has no db to write
  for (const WLayer& w : n->L)
    if (w.zb) return false;
  for (size_t l = 0; l + 1 < n->L.size(); ++l)
    if (n->L[l].act != ACT_SWISH && n->L[l].act != ACT_SIN) return false;
  if (n->L.back().act != ACT_NONE) return false;
  if (n->fc && n->pre_act != ACT_NONE) return false;
  return n->pre_act == ACT_NONE || n->pre_act == ACT_SWISH || n->pre_act == ACT_SIN;
}

float* grad_out(float* const* arr, int l) { return arr ? arr[l] : nullptr; }

// layer l's gradients from G_hd (against the tangent input) and G_h (against the primal input, may be null)
int layer_param_grads(InfNet* n, int l, const float* G_tan, const float* X_tan, const float* G_pri, const float* X_pri,
                      const float* X_pri_beta, const InfNetGrads* gr, int B, GradBufs& gb, hipStream_t s) {
  const WLayer& w = n->L[l];
  float* dW = grad_out(gr->dW, l);
  if (dW) {
    const long mn = (long)w.cout * w.cin * w.ks * w.ks;
    // the primal operand's swish once per element, not inside every output tile's loader
    if (G_pri && X_pri_beta) {
      INF_TRY(launch_act_apply(X_pri, ACT_SWISH, X_pri_beta, gb.act, (long)B * w.cin * n->P, s));
      X_pri = gb.act;
      X_pri_beta = nullptr;
    }
    if (G_tan) {
      INF_TRY(layer_wgrad(n, l, G_tan, X_tan, nullptr, gb.dWe, B, gb, s));
      if (G_pri) {
        INF_TRY(layer_wgrad(n, l, G_pri, X_pri, X_pri_beta, gb.dWe2, B, gb, s));
        INF_TRY(glue_add(gb.dWe2, gb.dWe, gb.dWe, mn, s));
      }
    } else {
      INF_TRY(layer_wgrad(n, l, G_pri, X_pri, X_pri_beta, gb.dWe, B, gb, s));
    }
    INF_TRY(layer_sigma_chain(n, l, gb.dWe, dW, gb, s));
  }
  float* db = grad_out(gr->db, l);
  if (db) {
    if (G_pri) INF_TRY(n->fc ? launch_channel_sum(G_pri, 1, w.cout, B, db, s) : launch_channel_sum(G_pri, B, w.cout, n->P, db, s));
    else INF_HIP(hipMemsetAsync(db, 0, sizeof(float) * w.cout, s));
  }
  return INF_OK;
}

// sum(gout * f(x)) differentiated into every parameter (and x, into gx when given) on internal-layout tensors: conv
// (B, C, H, W), fc (d, B)
int param_grad_core(InfNet* n, const float* x, const float* gout, float* gx, const InfNetGrads* gr, int B, GradBufs& gb,
                    hipStream_t s) {
  const int L = (int)n->L.size();
  const long hidP = (long)n->P;
  // forward: pre-activations (each layer's input activated once, gb.A)
  std::vector<const float*> Ain(L, nullptr);
  for (int l = 0; l < L; ++l) {
    INF_TRY(layer_input(n, l, x, gb, B, s, &Ain[l]));
    if (l + 1 < L) INF_TRY(layer_fwd(n, l, Ain[l], nullptr, true, gb.H[l], B, gb, s));
  }
  // backward
  const float* g = gout;
  float* bufs[2] = {gb.gA, gb.gB};
  for (int l = L - 1; l >= 0; --l) {
    INF_TRY(layer_param_grads(n, l, nullptr, nullptr, g, Ain[l], nullptr, gr, B, gb, s));
    if (l > 0) {
      const WLayer& prev = n->L[l - 1];
      const long ne = (long)B * prev.cout * hidP;
      INF_TRY(layer_vjp(n, l, g, gb.ga, B, gb, s));
      float* gp = bufs[l & 1];
      INF_TRY(launch_act_bwd1(gb.ga, gb.H[l - 1], prev.act, prev.act_beta, gp, gb.bpart, ne, GRAD_BLOCKS, s));
      float* dbeta = grad_out(gr->dbeta, l - 1);
      if (dbeta && prev.act == ACT_SWISH) INF_TRY(launch_beta_reduce(gb.bpart, GRAD_BLOCKS, dbeta, 0, s));
      g = gp;
    } else if (gx || (n->pre_beta && gr->dpre_beta)) {
      const long ne = (long)B * n->d;
      float* gin = gx ? gx : gb.tmp_in;
      if (n->pre_act != ACT_NONE) {     // a leading Swish (with its beta) or Sin
        INF_TRY(layer_vjp(n, 0, g, gb.ga, B, gb, s));
        INF_TRY(launch_act_bwd1(gb.ga, x, n->pre_act, n->pre_beta, gin, gb.bpart, ne, GRAD_BLOCKS, s));
        if (n->pre_beta && gr->dpre_beta) INF_TRY(launch_beta_reduce(gb.bpart, GRAD_BLOCKS, gr->dpre_beta, 0, s));
      } else {
        INF_TRY(layer_vjp(n, 0, g, gin, B, gb, s));
      }
    }
  }
  return INF_OK;
}

// s = sum_b w_b^T J(x_b) eps_b (w, eps fixed) differentiated into x (gx) and every parameter, forward-over-reverse, on
// internal-layout tensors; the per-sample value s_b (conv nets only: value non-null)
int surrogate_core(InfNet* n, const float* x, const float* w, const float* eps, float* value, float* gx,
                   const InfNetGrads* gr, int B, GradBufs& gb, hipStream_t s) {
  const int L = (int)n->L.size();
  const long nin = (long)B * n->d;
  // input tangent: eps * preact'(x) (or eps)
  const float* in_tan = eps;
  if (n->pre_act != ACT_NONE) {
    INF_HIP(hipMemcpyAsync(gb.Ad[0], eps, sizeof(float) * nin, hipMemcpyDeviceToDevice, s));
    INF_TRY(launch_act_tangent(gb.Ad[0], x, n->pre_act, n->pre_beta, nin, s));
    in_tan = gb.Ad[0];
  }
  // forward: primal pre-activations H, tangents Hd, activation tangents Ad
  std::vector<const float*> Ain(L, nullptr);     // each layer's input activated once (gb.A)
  for (int l = 0; l + 1 < L; ++l) {
    INF_TRY(layer_input(n, l, x, gb, B, s, &Ain[l]));
    INF_TRY(layer_fwd(n, l, Ain[l], nullptr, true, gb.H[l], B, gb, s));
    const float* tin = l == 0 ? in_tan : gb.Ad[l];
    INF_TRY(layer_fwd(n, l, tin, nullptr, false, gb.Hd[l], B, gb, s));
    const long ne = (long)B * n->L[l].cout * n->P;
    INF_HIP(hipMemcpyAsync(gb.Ad[l + 1], gb.Hd[l], sizeof(float) * ne, hipMemcpyDeviceToDevice, s));
    INF_TRY(launch_act_tangent(gb.Ad[l + 1], gb.H[l], n->L[l].act, n->L[l].act_beta, ne, s));
  }
  // reverse: G_tan = gbar of the layer's tangent output, G_pri = gbar of its primal output
  const float* G_tan = w;
  const float* G_pri = nullptr;
  float* tb[2] = {gb.gA, gb.gB};
  float* pb2[2] = {gb.hA, gb.hB};
  for (int l = L - 1; l >= 0; --l) {
    const float* X_tan = l == 0 ? in_tan : gb.Ad[l];
    if (!Ain[l]) INF_TRY(layer_input(n, l, x, gb, B, s, &Ain[l]));   // (the last layer's input)
    const float* X_pri = Ain[l];
    const float* xb = nullptr;
    INF_TRY(layer_param_grads(n, l, G_tan, X_tan, G_pri, X_pri, xb, gr, B, gb, s));
    INF_TRY(layer_vjp(n, l, G_tan, gb.gad, B, gb, s));
    if (G_pri) INF_TRY(layer_vjp(n, l, G_pri, gb.ga, B, gb, s));
    if (l == L - 1 && value) {
      // s_b = sum w . (W_{L-1} * adot_{L-2}) = sum (W_{L-1}^T w) . adot_{L-2}
      const long per = (long)n->L[l].cin * n->P;
      INF_TRY(glue_batched_dot(gb.gad, X_tan, value, B, per, gb.bpart, s));
    }
    if (l > 0) {
      const WLayer& prev = n->L[l - 1];
      const long ne = (long)B * prev.cout * n->P;
      float* nt = tb[l & 1];
      float* np = pb2[l & 1];
      INF_TRY(launch_act_bwd2(gb.gad, G_pri ? gb.ga : nullptr, gb.H[l - 1], gb.Hd[l - 1], prev.act, prev.act_beta, nt,
                              np, gb.bpart, ne, GRAD_BLOCKS, s));
      float* dbeta = grad_out(gr->dbeta, l - 1);
      if (dbeta && prev.act == ACT_SWISH) INF_TRY(launch_beta_reduce(gb.bpart, GRAD_BLOCKS, dbeta, 0, s));
      G_tan = nt;
      G_pri = np;
    } else {
      float* gin = gx ? gx : gb.tmp_in;
      if (n->pre_act != ACT_NONE) {
        // x-gradient: gbar_adot eps s''(x) + gbar_a s'(x); beta: ... (act_bwd2 with h = x, hdot = eps)
        INF_TRY(launch_act_bwd2(gb.gad, G_pri ? gb.ga : nullptr, x, eps, n->pre_act, n->pre_beta, gb.xin, gin, gb.bpart,
                                nin, GRAD_BLOCKS, s));
        if (n->pre_beta && gr->dpre_beta) INF_TRY(launch_beta_reduce(gb.bpart, GRAD_BLOCKS, gr->dpre_beta, 0, s));
      } else if (gx) {
        if (G_pri) INF_HIP(hipMemcpyAsync(gx, gb.ga, sizeof(float) * nin, hipMemcpyDeviceToDevice, s));
        else INF_HIP(hipMemsetAsync(gx, 0, sizeof(float) * nin, s));
      }
    }
  }
  return INF_OK;
}

// ---- the log-det estimators' gradients for fc nets (the training path of train_tabular.py / train_toy.py) -----------
constexpr int FC_JAC_MAX = 16;     // widest fc net with an explicit per-sample Jacobian (fc_jacobian, logdet_pairs_kernel)

// b_scr: the wide series' forward-tangent chain (n_terms + 1, d, B); d <= FC_JAC_MAX takes nothing for it
size_t logdet_grad_layout(InfNet* n, int B, int mode, int n_terms, char* ws, size_t cap, Bufs* bf, GradBufs* gb,
                          float** A, float** bv, float** xr, float** gxs, float** eps_t, float** a_scr, float** b_scr) {
  const int T = mode == LOGDET_SERIES ? n_terms : n->d;
  const long N = (long)T * B;
  Bufs bf0;
  GradBufs gb0;
  const size_t s1 = (carve(n, B, 1, ws, ws ? cap : 0, bf ? *bf : bf0) + 255) & ~(size_t)255;
  char* w2 = ws ? ws + s1 : nullptr;
  const size_t s2 = (carve_grad(n, (int)N, w2, ws ? (cap > s1 ? cap - s1 : 0) : 0, gb ? *gb : gb0) + 255) & ~(size_t)255;
  WS w{ws ? ws + s1 + s2 : nullptr, ws ? (cap > s1 + s2 ? cap - s1 - s2 : 0) : 0, 0};
  float* p[6];
  // (eps_t: the Jacobian route's transposed probes; the wide route transposes them straight into a_scr)
  const size_t cnt[6] = {(size_t)n->d * N, (size_t)n->d * N, (size_t)n->d * N, (size_t)n->d * N,
                         n->d > FC_JAC_MAX ? 0 : (size_t)n->d * B, mode == LOGDET_SERIES ? (size_t)n_terms * n->d * B : 1};
  for (int i = 0; i < 6; ++i) p[i] = w.take<float>(cnt[i]);
  float* pb = n->d > FC_JAC_MAX ? w.take<float>(((size_t)n_terms + 1) * n->d * B) : nullptr;
  if (A) {
    *A = p[0];
    *bv = p[1];
    *xr = p[2];
    *gxs = p[3];
    *eps_t = p[4];
    *a_scr = p[5];
    *b_scr = pb;
  }
  return s1 + s2 + w.off + 256;
}

// v -> J(x) v on internal-layout tensors: the forward-tangent chain on the per-layer GEMMs, the hidden layers' tangents
// scaled by the activation derivatives run_forward(mode = -1) saved at x (bf.D), the last layer stored into out
int run_jvp(InfNet* n, const float* v, float* out, int B, Bufs& bf, hipStream_t s) {
  const int L = (int)n->L.size();
  const float* cur = v;
  for (int l = 0; l < L; ++l) {
    const WLayer& w = n->L[l];
    const bool last = l == L - 1;
    float* o = last ? out : ((l % 2 == 0) ? bf.h0 : bf.h1);
    GemmArgs g = gemm_base(n, w.f, cur, w.cin, B);
    set_out(n, g, o, w.cout);
    g.deriv_in = last ? nullptr : bf.D[l];
    INF_TRY(layer_gemm(n, g, w.f.load, last ? EP_STORE : EP_MUL_DERIV, bf.kslab, bf.kslab_bytes, s));
    cur = o;
  }
  return INF_OK;
}

// The series' pairs without a Jacobian (fc nets wider than FC_JAC_MAX): a_j = (J^T)^j eps by the VJP chain the series
// value runs (a_scr, j < n), b_m = J^m eps by the forward-tangent chain (b_scr, m <= n: b_n only enters the value), then
// series_pairs_wide_kernel stacks A, bv, xr over the n B columns and writes the value.  Leaves x internal in bf.xin.
int series_pairs_chains(InfNet* n, const float* x, const float* eps, const float* coeff, int n_terms, const float* gout,
                        float* value, int B, Bufs& bf, float* A, float* bv, float* xr, float* a_scr, float* b_scr,
                        hipStream_t s) {
  const size_t dB = (size_t)n->d * B;
  const float* xi;
  INF_TRY(to_internal(n, x, bf.xin, B, s, &xi));
  INF_TRY(launch_transpose(eps, a_scr, B, n->d, s));
  INF_HIP(hipMemcpyAsync(b_scr, a_scr, sizeof(float) * dB, hipMemcpyDeviceToDevice, s));
  INF_TRY(run_forward(n, xi, B, bf, -1, nullptr, s));
  for (int j = 0; j + 1 < n_terms; ++j)
    INF_TRY(run_vjp(n, a_scr + j * dB, a_scr + (j + 1) * dB, xi, nullptr, nullptr, B, bf, s));
  for (int m = 0; m < n_terms; ++m) INF_TRY(run_jvp(n, b_scr + m * dB, b_scr + (m + 1) * dB, B, bf, s));
  return launch_series_pairs_wide(a_scr, b_scr, xi, gout, coeff, n_terms, n->d, B, A, bv, xr, value, s);
}

}  // namespace

extern "C" {

size_t inf_grad_workspace_bytes(InfNet* n, int B) {
  if (!n || B <= 0) return 0;
  GradBufs gb;
  return carve_grad(n, B, nullptr, 0, gb);
}

// Gradient of sum(gout * f(x)) with respect to every parameter of the net (and x): the recompute graph of the training
// forward (implicit_block.py:226-227) and the first-order terms of any caller.  Conv and fc nets with Swish / Sin
// (grad_supported); fc nets: x, gout, gx in the (B, d) boundary layout.
int inf_net_param_grad(InfNet* n, const float* x, const float* gout, float* gx, const InfNetGrads* gr, int B,
                       void* ws, size_t ws_bytes, void* stream) {
  if (!n || !x || !gout || !gr || B <= 0) return INF_ERR_INVALID;
  if (!grad_supported(n)) return INF_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  GradBufs gb;
  if (!ws || carve_grad(n, B, ws, ws_bytes, gb) > ws_bytes) return INF_ERR_WORKSPACE;
  if (!n->fc) return param_grad_core(n, x, gout, gx, gr, B, gb, s);
  INF_TRY(launch_transpose(x, gb.x_t, B, n->d, s));
  INF_TRY(launch_transpose(gout, gb.w_t, B, n->d, s));
  INF_TRY(param_grad_core(n, gb.x_t, gb.w_t, gx ? gb.gx_t : nullptr, gr, B, gb, s));
  if (gx) INF_TRY(launch_transpose(gb.gx_t, gx, n->d, B, s));
  return INF_OK;
}

// Gradient of s = sum_b w_b^T J(x_b) eps_b (w fixed) with respect to x and every parameter, and the value s_b per
// sample (conv nets): the memory-efficient Neumann estimator's surrogate (implicit_block.py:388-394,437-438),
// forward-over-reverse on the engine.  fc nets: x, w, eps, gx in the (B, d) boundary layout, value NULL.
int inf_net_surrogate_grad(InfNet* n, const float* x, const float* w, const float* eps, float* value, float* gx,
                           const InfNetGrads* gr, int B, void* ws, size_t ws_bytes, void* stream) {
  if (!n || !x || !w || !eps || !gr || B <= 0) return INF_ERR_INVALID;
  if (!grad_supported(n) || (n->fc && value)) return INF_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  GradBufs gb;
  if (!ws || carve_grad(n, B, ws, ws_bytes, gb) > ws_bytes) return INF_ERR_WORKSPACE;
  if (!n->fc) return surrogate_core(n, x, w, eps, value, gx, gr, B, gb, s);
  INF_TRY(launch_transpose(x, gb.x_t, B, n->d, s));
  INF_TRY(launch_transpose(w, gb.w_t, B, n->d, s));
  INF_TRY(launch_transpose(eps, gb.e_t, B, n->d, s));
  INF_TRY(surrogate_core(n, gb.x_t, gb.w_t, gb.e_t, nullptr, gx ? gb.gx_t : nullptr, gr, B, gb, s));
  if (gx) INF_TRY(launch_transpose(gb.gx_t, gx, n->d, B, s));
  return INF_OK;
}

size_t inf_logdet_grad_workspace_bytes(InfNet* n, int B, int mode, int n_terms) {
  if (!n || B <= 0 || mode < LOGDET_SERIES || mode > LOGDET_TRACE || (mode != LOGDET_EXACT && n_terms < 1)) return 0;
  return logdet_grad_layout(n, B, mode, n_terms, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                            nullptr, nullptr, nullptr);
}

// g . S(x) differentiated into every parameter of an fc net and into x, S_b one of the log-det estimators of a sample
// (mode INF_LOGDET_SERIES / EXACT / TRACE): the estimator's bilinear pairs at x, then one forward-over-reverse pass over
// the T B stacked pairs (surrogate_core: the GEMM chains of the generic path, N = T B columns), the x-gradient summed
// over each sample's pairs.  d <= 16: the pairs from the Jacobian per sample (fc_jacobian, logdet_est.hip
// logdet_pairs_kernel).  Wider nets, the series only: from the VJP and forward-tangent chains (series_pairs_chains); the
// exact log-det and the exact trace need the Jacobian and stay INF_ERR_UNSUPPORTED.
int inf_logdet_grad(InfNet* n, const float* x, int mode, const float* eps, const float* coeff, int n_terms,
                    const float* gout, float* value, float* gx, const InfNetGrads* gr, int B, void* ws, size_t ws_bytes,
                    void* stream) {
  if (!n || !x || !gr || B <= 0 || mode < LOGDET_SERIES || mode > LOGDET_TRACE) return INF_ERR_INVALID;
  if (mode == LOGDET_SERIES && (!eps || !coeff || n_terms < 1 || n_terms > 128)) return INF_ERR_INVALID;
  if (mode == LOGDET_TRACE && (!coeff || n_terms < 1 || n_terms > 128)) return INF_ERR_INVALID;
  const bool wide = n->fc && n->d > FC_JAC_MAX;
  if (!n->fc || (wide && mode != LOGDET_SERIES) || !grad_supported(n)) return INF_ERR_UNSUPPORTED;
  if (wide && (long)n_terms * B > 0x7fffffffL) return INF_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  Bufs bf;
  GradBufs gb;
  float *A, *bv, *xr, *gxs, *eps_t, *a_scr, *b_scr;
  const int nt = mode == LOGDET_EXACT ? 1 : n_terms;
  if (!ws || logdet_grad_layout(n, B, mode, nt, reinterpret_cast<char*>(ws), ws_bytes, &bf, &gb, &A, &bv, &xr, &gxs,
                                &eps_t, &a_scr, &b_scr) > ws_bytes)
    return INF_ERR_WORKSPACE;
  const int T = mode == LOGDET_SERIES ? n_terms : n->d;
  if (wide) {
    INF_TRY(series_pairs_chains(n, x, eps, coeff, n_terms, gout, value, B, bf, A, bv, xr, a_scr, b_scr, s));
  } else {
    const float* tang = nullptr;
    INF_TRY(fc_jacobian(n, x, B, bf, &tang, s));                     // also leaves x internal in bf.xin
    if (mode == LOGDET_SERIES) INF_TRY(launch_transpose(eps, eps_t, B, n->d, s));
    const float one = 1.f;
    INF_TRY(launch_logdet_pairs(mode, tang, eps_t, bf.xin, gout, mode == LOGDET_EXACT ? &one : coeff, nt, n->d, B, A,
                                bv, xr, value, a_scr, s));
  }
  INF_TRY(surrogate_core(n, xr, A, bv, nullptr, gx ? gxs : nullptr, gr, T * B, gb, s));
  if (gx) INF_TRY(launch_sum_pairs(gxs, T, n->d, B, gx, s));
  return INF_OK;
}

}  // extern "C"
