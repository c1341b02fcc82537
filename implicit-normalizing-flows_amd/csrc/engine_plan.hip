// Net plans: what a net is (its layers, operands and device storage), its per-net options, and how a caller's workspace
// is carved for it.
//
// Reference mapping:
//   inf_net_create        <- the nn.Sequential of InducedNorm layers + activations that ImplicitFlow builds
//                            (implicit_flow.py:371-373 for the leading activation)
//   inf_net_refresh       <- InducedNorm*.compute_weight(update=False) (mixed_lipschitz.py:126-132,267-386)
//   inf_net_set_tensors   <- a DataParallel replica's parameter copies (train_img.py:203-204,820)
#include <memory>
#include <new>

#include "engine.h"

using namespace inf;

namespace {

int round_up(int x, int m) { return (x + m - 1) / m * m; }

// the activations the fused 3-1-3 conv kernels have a form for (fused313*.hip)
bool fused_act_kind(int act) {
  return act == ACT_SWISH || act == ACT_SIN || act == ACT_ELU || act == ACT_SOFTPLUS || act == ACT_RELU;
}

// InfLayerKind of an activation -> Act, or -1 for any other kind
int act_of_kind(int kind) {
  switch (kind) {
    case INF_ACT_SWISH: return ACT_SWISH;
    case INF_ACT_SIN: return ACT_SIN;
    case INF_ACT_ELU: return ACT_ELU;
    case INF_ACT_SOFTPLUS: return ACT_SOFTPLUS;
    case INF_ACT_RELU: return ACT_RELU;
    case INF_ACT_LCUBE: return ACT_LCUBE;
    case INF_ACT_IDENTITY: return ACT_IDENTITY;
    case INF_ACT_ZERO: return ACT_ZERO;
    default: return -1;
  }
}

// Element counts of a fused 3-1-3 net's six operands, in F1f..F3b order (create's accounting and pointer layout,
// refresh's split launches)
struct FusedSizes {
  size_t n[6];
  explicit FusedSizes(const InfNet* net) {
    n[0] = n[1] = (size_t)net->fhid * net->K1pad;
    n[2] = n[3] = (size_t)net->fhid * net->fhid;
    n[4] = n[5] = (size_t)net->M3pad * net->fhid;
  }
  size_t sum() const { return n[0] + n[1] + n[2] + n[3] + n[4] + n[5]; }
};

// INFLOW_MFMA ("f32" / "fp32" / "bf16x6" / "f16x3"; unset or empty: *mode stays) -> *mode.  has_bf16x6: the conv kernels;
// the fc kernels have no bf16x6 variant and bf16x6 selects exact fp32 for them.
int parse_mfma(const char* mm, bool has_bf16x6, int* mode) {
  if (!mm || !*mm) return INF_OK;
  if (!strcmp(mm, "f32") || !strcmp(mm, "fp32")) *mode = INF_MFMA_F32;
  else if (!strcmp(mm, "bf16x6")) *mode = has_bf16x6 ? INF_MFMA_BF16X6 : INF_MFMA_F32;
  else if (strcmp(mm, "f16x3") != 0) {
    fprintf(stderr, "libinflow: INFLOW_MFMA=%s is not one of f32, fp32, bf16x6, f16x3\n", mm);
    return INF_ERR_INVALID;
  }
  return INF_OK;
}

// The per-net options: inf_net_create's environment defaults, inf_net_set_option and inf_net_get_option all read this
// table.  names: the values the environment variable accepts, the value being the index.
struct NetOption {
  int id;
  int InfNet::*slot;
  int hi;                 // highest valid value
  const char* env;        // default read at inf_net_create, or null
  const char* names[4];
  bool resets_f0;         // a kernel-variant option changes the bits of f(0): the cached value is recomputed on next use
};
const NetOption OPTIONS[] = {
    {INF_OPT_FUSED_K128, &InfNet::k128, 3, "INFLOW_FUSED_K128", {"0", "1", "2", "3"}, true},
    {INF_OPT_EVAL_OVERLAP, &InfNet::eval_overlap, 1, "INFLOW_EVAL_OVERLAP", {"0", "1"}, false},
    {INF_OPT_CONVERGENCE, &InfNet::convergence, 1, "INFLOW_CONVERGENCE", {"global", "per_sample"}, false},
    {INF_OPT_LINE_SEARCH, &InfNet::line_search, 1, nullptr, {}, false},
    {INF_OPT_K128_EXACT_SCALE, &InfNet::exact_scale, 1, nullptr, {}, true},
    {INF_OPT_FC_BLOCK, &InfNet::fc_block, 2, "INFLOW_FC_BLOCK", {"0", "1", "2"}, false},
    {INF_OPT_FC_SERIES, &InfNet::fc_series, 1, "INFLOW_FC_SERIES", {"0", "1"}, false},
    {INF_OPT_FC_SKINNY, &InfNet::fc_skinny, 1, nullptr, {}, false},
    {INF_OPT_FUSED_PRESPLIT, &InfNet::presplit, 1, "INFLOW_FUSED_PRESPLIT", {"0", "1"}, false},
    {INF_OPT_SERIES_GROUP, &InfNet::series_group, INF_SERIES_GROUP_OFF, nullptr, {}, false},
};
const NetOption* find_option(int id) {
  for (const NetOption& o : OPTIONS)
    if (o.id == id) return &o;
  return nullptr;
}

void free_net(InfNet* n) {
  if (!n) return;
  if (n->dev) (void)hipFree(n->dev);
  if (n->scratch) (void)hipFree(n->scratch);
  if (n->f0) (void)hipFree(n->f0);
  if (n->fch) (void)hipFree(n->fch);
  if (n->fchexp) (void)hipFree(n->fchexp);
  delete n;
}
struct NetDeleter {
  void operator()(InfNet* n) const { free_net(n); }
};

// (a fused net's d1 / d2 are in fragment order per tile: hidden x tiles x tile width floats, dead columns included)
size_t per_sample_hidden(const InfNet* n) {
  return (size_t)n->hidden_max * (n->fc ? 1 : (n->fused ? std::max(n->P, n->fpix) : n->P));
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// workspace carving
// ---------------------------------------------------------------------------------------------
// layout-aware sizes: E = B * d elements per vector
size_t inf::carve(const InfNet* n, int B, int T, void* ws, size_t cap, Bufs& b) {
  WS w{reinterpret_cast<char*>(ws), cap, 0};
  const size_t E = (size_t)B * n->d;
  const size_t Hs = (size_t)B * per_sample_hidden(n);
  const size_t Ys = (size_t)B * n->rows_max * (n->fc ? 1 : n->P);
  // (narrow fc nets: one partial per sample; wide fc nets and conv nets: one per OUT_CH-element chunk)
  const int nchunk = n->fc ? fc_nchunk(n->d) : out_nchunk(n->d);
  b.nchunk = nchunk;
  b.snchunk = n->fused ? std::max(nchunk, std::max(n->P / 32, n->ftiles)) : nchunk;
  b.h0 = w.take<float>(Hs);
  b.h1 = w.take<float>(Hs);
  b.Y = w.take<float>(Ys);
  b.Y2 = n->fused ? w.take<float>(Ys) : nullptr;
  b.D.resize(n->L.size() > 0 ? n->L.size() - 1 : 0);
  for (auto& p : b.D) p = w.take<float>(Hs);
  float** vecs[] = {&b.xin, &b.xemb, &b.fx, &b.xa, &b.xb, &b.ga, &b.gb, &b.upd,
                    &b.dx, &b.dg, &b.lowest, &b.va, &b.vb, &b.eps_t, &b.zero, &b.tmp, &b.fcur, &b.flow,
                    &b.fspec, &b.ps_lowx, &b.ps_lowf};
  for (float** v : vecs) *v = w.take<float>(E);
  b.U = w.take<float>((size_t)T * E);
  b.VT = w.take<float>((size_t)T * E);
  if (n->fc && n->d <= 16) {   // forward-mode tangents (fc_jacobian): every user declines d > 16
    const size_t ext = (size_t)(n->d + 1) * B * std::max(n->hidden_max, n->d);
    b.ext0 = w.take<float>(ext);
    b.ext1 = w.take<float>(ext);
  } else {
    b.ext0 = b.ext1 = nullptr;
  }
  b.part = w.take<double>((size_t)B * std::max(nchunk, b.snchunk) * SERIES_MAX);
  const int bch = (n->d + 1023) / 1024;
  b.bpart = w.take<double>((size_t)B * bch * (3 * (size_t)T + 2) + 64);
  b.sumsq = w.take<double>((size_t)B + 1);
  b.counter = w.take<unsigned int>(64);
  b.ps_state = w.take<double>((size_t)B * (PS_HEAD + T));
  b.ps_active = w.take<int>((size_t)B);
  b.ps_improved = w.take<int>((size_t)B);
  if (n->fc) {
    b.bk_sync_bytes = 16 + sizeof(unsigned long long) * 8 * (size_t)fcblock_grid(B);   // 4 sets x 2 granules
    b.bk_sync = reinterpret_cast<unsigned*>(w.take<char>(b.bk_sync_bytes));
    b.bk_out_bytes = sizeof(FcBlockStats) + (sizeof(int) * 3 + sizeof(double)) * (size_t)B + 64;
    b.bk_out = w.take<char>(b.bk_out_bytes);
  } else {
    b.bk_sync = nullptr;
    b.bk_out = nullptr;
    b.bk_sync_bytes = b.bk_out_bytes = 0;
  }
  // (carved whatever INF_OPT_FC_SKINNY says: a workspace sized before the option changes stays large enough)
  b.kslab_bytes = (n->fc && n->d > FC_NARROW_MAX) ? SKINNY_SLAB_BYTES : 0;
  b.kslab = b.kslab_bytes ? w.take<float>(b.kslab_bytes / sizeof(float)) : nullptr;
  return w.off + 256;
}

size_t inf::ws_need(const InfNet* n, int B, int T) {
  Bufs b;
  return carve(n, B, T, nullptr, 0, b);
}

extern "C" {

size_t inf_workspace_bytes(const InfNet* n, int batch, int threshold) {
  if (!n || batch <= 0) return 0;
  return ws_need(n, batch, std::max(threshold, 1));
}

// Re-points a net at other tensors of the same layout (a DataParallel replica's copies of the parameters on another
// device, lib/_hip native_net): the pointers the refresh and the launches read change, nothing is repacked -- the caller
// refreshes only when the values differ from the last refresh's.
int inf_net_set_tensors(InfNet* n, const InfNetDesc* desc) {
  if (!n || !desc || desc->n_layers <= 0 || !desc->layers) return INF_ERR_INVALID;
  int i = 0;
  const int pre_kind = act_of_kind(desc->layers[0].kind);
  const bool pre = pre_kind >= 0;
  if ((pre ? pre_kind : (int)ACT_NONE) != n->pre_act) return INF_ERR_INVALID;
  if (pre) i = 1;
  size_t l = 0;
  std::vector<WLayer> L = n->L;
  const float* pre_beta = n->pre_act == ACT_SWISH ? desc->layers[0].beta : nullptr;
  if (n->pre_act == ACT_SWISH && !pre_beta) return INF_ERR_INVALID;
  for (; i < desc->n_layers; ++i) {
    const InfLayerDesc& d = desc->layers[i];
    if (d.kind == INF_LAYER_CONV || d.kind == INF_LAYER_LINEAR) {
      if (l >= L.size()) return INF_ERR_INVALID;
      WLayer& w = L[l++];
      const int ks = d.kind == INF_LAYER_LINEAR ? 1 : d.ksize;
      if (w.kind != d.kind || w.cin != d.cin || w.cout != d.cout || w.ks != ks || !d.weight || !d.u || !d.v)
        return INF_ERR_INVALID;
      if ((d.bias == nullptr) != (w.zb != nullptr)) return INF_ERR_INVALID;   // bias-free layers stay bias-free
      w.W = d.weight;
      w.b = d.bias ? d.bias : w.zb;
      w.u = d.u;
      w.v = d.v;
    } else if (act_of_kind(d.kind) >= 0) {
      if (l == 0 || L[l - 1].act != act_of_kind(d.kind)) return INF_ERR_INVALID;
      if (d.kind == INF_ACT_SWISH && !d.beta) return INF_ERR_INVALID;
      L[l - 1].act_beta = d.kind == INF_ACT_SWISH ? d.beta : nullptr;
    } else {
      return INF_ERR_INVALID;
    }
  }
  if (l != L.size()) return INF_ERR_INVALID;
  n->L = L;
  n->pre_beta = pre_beta;
  return INF_OK;
}

// The net is owned by `net` until the last line: every failure is a plain return, and what was allocated by then goes
// the way inf_net_destroy frees it.
int inf_net_create(const InfNetDesc* desc, InfNet** out) {
  if (!desc || !out || desc->n_layers <= 0 || !desc->layers) return INF_ERR_INVALID;
  std::unique_ptr<InfNet, NetDeleter> net(new (std::nothrow) InfNet());
  InfNet* n = net.get();
  if (!n) return INF_ERR_INVALID;
  n->C = desc->channels;
  n->H = desc->height;
  n->W = desc->width;
  n->P = n->H * n->W;
  n->d = n->C * n->P;
  int i = 0;
  // leading activation (preact, implicit_flow.py:371-373)
  // (pre_beta is set for a leading Swish only; the kernels read the kind of any other from pre_act)
  if (act_of_kind(desc->layers[0].kind) >= 0) {
    n->pre_act = act_of_kind(desc->layers[0].kind);
    n->pre_beta = n->pre_act == ACT_SWISH ? desc->layers[0].beta : nullptr;
    if (n->pre_act == ACT_SWISH && !n->pre_beta) return INF_ERR_INVALID;
    i = 1;
  }
  for (; i < desc->n_layers; ++i) {
    const InfLayerDesc& d = desc->layers[i];
    if (d.kind == INF_LAYER_CONV || d.kind == INF_LAYER_LINEAR) {
      WLayer w;
      w.kind = d.kind;
      w.cin = d.cin;
      w.cout = d.cout;
      w.ks = d.kind == INF_LAYER_LINEAR ? 1 : d.ksize;
      w.W = d.weight;
      w.b = d.bias;
      w.u = d.u;
      w.v = d.v;
      w.coeff = d.coeff;
      if (w.ks != 1 && w.ks != 3) return INF_ERR_UNSUPPORTED;
      n->L.push_back(w);
    } else if (act_of_kind(d.kind) >= 0) {
      if (n->L.empty() || n->L.back().act != ACT_NONE) return INF_ERR_UNSUPPORTED;
      if (d.kind == INF_ACT_SWISH && !d.beta) return INF_ERR_INVALID;
      n->L.back().act = act_of_kind(d.kind);
      n->L.back().act_beta = d.kind == INF_ACT_SWISH ? d.beta : nullptr;
    } else {
      return INF_ERR_INVALID;
    }
  }
  const int L = (int)n->L.size();
  if (L == 0 || n->L.back().act != ACT_NONE) return INF_ERR_UNSUPPORTED;
  // A leading activation other than Swish is applied by the GEMM loader of the instantiations that carry it: a leading
  // Sin by EP_ACT_SIN's (the first layer's activation is Sin), any other by the parameter-less family's own (gemm.hip
  // EP_ACT_ANY: the first layer's activation is of that family too) -- every net ImplicitFlow builds (one activation_fn
  // throughout).  Other mixes are not implemented.
  if (n->pre_act != ACT_NONE && n->pre_act != ACT_SWISH) {
    const int a0 = n->L[0].act;
    const bool ok = n->pre_act == ACT_SIN ? a0 == ACT_SIN : (a0 != ACT_NONE && a0 != ACT_SWISH && a0 != ACT_SIN);
    if (!ok) return INF_ERR_UNSUPPORTED;
  }
  n->fc = n->L[0].kind == INF_LAYER_LINEAR;
  if (n->fc) {
    n->d = n->C;
    n->P = 1;
  }
  // channel chain: C -> ... -> C
  int ch = n->C;
  for (auto& w : n->L) {
    if (w.cin != ch || (n->fc && w.kind != INF_LAYER_LINEAR) || (!n->fc && w.kind != INF_LAYER_CONV))
      return INF_ERR_UNSUPPORTED;
    ch = w.cout;
  }
  if (ch != n->C) return INF_ERR_UNSUPPORTED;
  // plans
  size_t floats = 0;
  for (int l = 0; l < L; ++l) {
    WLayer& w = n->L[l];
    const bool last = l == L - 1, first = l == 0;
    if (l < L - 1) n->hidden_max = std::max(n->hidden_max, w.cout);
    // forward operand
    if (w.ks == 1) {
      w.f = Operand{BL_DIRECT, 0, w.cout, 0, w.cin, 0, PK_ROWMAJOR, nullptr};
    } else if (last && w.cout < TAPS_MAX_CH) {
      w.f = Operand{BL_DIRECT, 1, 9 * w.cout, 0, w.cin, 0, PK_TAPS_FWD, nullptr};
    } else {
      w.f = Operand{BL_IM2COL3, 0, w.cout, 0, 9 * w.cin, 0, PK_IM2COL_FWD, nullptr};
    }
    if (!last && w.f.taps) return INF_ERR_UNSUPPORTED;
    // vjp operand (maps grad wrt output -> grad wrt input)
    if (w.ks == 1) {
      w.g = Operand{BL_DIRECT, 0, w.cin, 0, w.cout, 0, PK_TRANSPOSE, nullptr};
    } else if (first && w.cin < TAPS_MAX_CH) {
      w.g = Operand{BL_DIRECT, 1, 9 * w.cin, 0, w.cout, 0, PK_TAPS_BWD, nullptr};
    } else {
      w.g = Operand{BL_IM2COL3, 0, w.cin, 0, 9 * w.cout, 0, PK_IM2COL_BWD, nullptr};
    }
    for (Operand* op : {&w.f, &w.g}) {
      op->Mpad = round_up(op->M, 128);
      op->Kpad = round_up(op->K, 16);
      floats += (size_t)op->Mpad * op->Kpad + 64;
    }
    floats += 64;   // factor
    if (!w.b) floats += (size_t)round_up(w.cout, 64);   // the zero bias of a bias-free layer
    if (last) n->rows_max = std::max(n->rows_max, w.f.M);
    if (first) n->rows_max = std::max(n->rows_max, w.g.M);
  }
  if (L == 1) n->hidden_max = std::max(n->hidden_max, 1);
  const char* no_fused = getenv("INFLOW_NO_FUSED");
  const bool fused_off = no_fused && no_fused[0] == '1';
  // fused fc net (fcnet.hip): 128-wide hidden layers with one activation kind, no input pre-activation
  {
    bool ok = n->fc && n->pre_act == ACT_NONE && L >= 2 && L <= FC_MAXL && !fused_off;
    for (int l = 0; ok && l < L; ++l) {
      const WLayer& w = n->L[l];
      if (l < L - 1 && (w.cout != 128 || w.act != n->L[0].act)) ok = false;
    }
    if (ok) {
      FcArgs f;
      memset(&f, 0, sizeof(f));
      f.nl = L;
      f.d = n->d;
      f.act = n->L[0].act;
      for (int l = 0; l < L; ++l) f.L[l].Kpad = n->L[l].f.Kpad;
      n->fcfused = fcnet_supported(f, false) != 0;
    }
    if (n->fcfused) {
      // f16x3 planes (fcnet_h3.hip): the input layer 8 row tiles x 1 k step, hidden 8 x 4, output 1 x 4; fragment tiles
      // of 2 x 512 halves.  The fused fc kernels default to f16x3 (INFLOW_MFMA=f32 / fp32: exact fp32 MFMA)
      size_t halves = 0;
      for (int l = 0; l < L; ++l) {
        n->fch_off.push_back(halves);
        const int nrt = l == L - 1 ? 1 : 8, nks = l == 0 ? 1 : 4;
        halves += (size_t)nrt * nks * 1024;
      }
      if (hipMalloc(&n->fch, 2 * halves * sizeof(uint16_t)) != hipSuccess ||
          hipMalloc(&n->fchexp, 2 * (size_t)L * sizeof(int)) != hipSuccess)
        return INF_ERR_HIP;
      n->fcht = n->fch + halves;            // one allocation each: freed with fch / fchexp
      n->fchtexp = n->fchexp + L;
      n->mfma_mode = INF_MFMA_F16X3;
      INF_TRY(parse_mfma(getenv("INFLOW_MFMA"), false, &n->mfma_mode));
    }
  }
  // fused 3-1-3 conv net (run_cifar10.sh nets): 3x3 C->H, swish, 1x1 H->H, swish, 3x3 H->C
  {
    const bool shape_ok = !n->fc && L == 3 && n->L[0].ks == 3 && n->L[1].ks == 1 && n->L[2].ks == 3 &&
                          fused_act_kind(n->L[0].act) && n->L[1].act == n->L[0].act &&
                          (n->pre_act == ACT_NONE || n->pre_act == n->L[0].act) &&
                          n->L[0].cout == n->L[1].cin && n->L[1].cin == n->L[1].cout && n->L[1].cout == n->L[2].cin;
    if (shape_ok && !fused_off && net313_supported(n->L[1].cout, n->C, n->H, n->W)) {
      n->fused = true;
      n->fhid = n->L[1].cout;
      n->ftiles = net313_max_tiles(n->fhid, n->C, n->H, n->W);
      n->fpix = net313_tile_pixels(n->fhid, n->C, n->H, n->W);
      n->K1pad = round_up(9 * n->C, 16);
      n->M3 = 9 * n->C;
      n->M3pad = round_up(9 * n->C, 32);
      const FusedSizes sz(n);
      floats += sz.sum() + 6 * 64;
      // split planes: 3 bf16 (= 1.5 floats) per element of each of the six operands
      floats += 3 * sz.sum() / 2 + 6 * 64;
      // F16X3 planes: 2 fp16 (= 1 float) per element of each of the six operands, plus the scale exponents
      floats += sz.sum() + 6 * 64 + 64;
      floats += sz.n[4] + sz.n[5] + 2 * 64;   // the permuted phase-C planes Fhp
      n->rows_max = std::max(n->rows_max, n->M3);
      n->mfma_mode = INF_MFMA_F16X3;
      INF_TRY(parse_mfma(getenv("INFLOW_MFMA"), true, &n->mfma_mode));
    }
  }
  // defaults of the per-net options; an unrecognised value fails inf_net_create (as INFLOW_MFMA does) rather
  // than silently selecting another rule
  for (const NetOption& o : OPTIONS) {
    const char* e = o.env ? getenv(o.env) : nullptr;
    if (!e || !*e) continue;
    int v = -1;
    for (int k = 0; k <= o.hi; ++k)
      if (!strcmp(e, o.names[k])) v = k;
    if (v < 0) {
      fprintf(stderr, "libinflow: %s=%s is not one of", o.env, e);
      for (int k = 0; k <= o.hi; ++k) fprintf(stderr, " %s", o.names[k]);
      fprintf(stderr, "\n");
      return INF_ERR_INVALID;
    }
    n->*o.slot = v;
  }
  // sigma scratch: one partial per 256 output elements of the largest conv (or per channel-split block)
  size_t sc = SIGMA_MAX_PARTS + 64;
  for (auto& w : n->L) sc = std::max(sc, (size_t)w.cout * (n->fc ? 1 : n->P) / 256 + 64);
  n->scratch_doubles = sc;
  if (hipGetDevice(&n->device) != hipSuccess) n->device = 0;
  if (hipMalloc(&n->dev, floats * sizeof(float)) != hipSuccess ||
      hipMalloc(&n->scratch, sc * sizeof(double)) != hipSuccess)
    return INF_ERR_HIP;
  float* p = n->dev;
  for (auto& w : n->L) {
    for (Operand* op : {&w.f, &w.g}) {
      op->A = p;
      p += (size_t)op->Mpad * op->Kpad + 64;
    }
    w.factor = p;
    p += 64;
    if (!w.b) {
      w.zb = p;
      w.b = p;
      p += round_up(w.cout, 64);
    }
  }
  if (n->fused) {
    float** bufs[] = {&n->F1f, &n->F1b, &n->F2f, &n->F2b, &n->F3f, &n->F3b};
    const FusedSizes sz(n);
    for (int k = 0; k < 6; ++k) {
      *bufs[k] = p;
      p += sz.n[k] + 64;
    }
    for (int k = 0; k < 6; ++k) {
      n->Fs[k] = reinterpret_cast<uint16_t*>(p);
      p += (3 * sz.n[k] + 1) / 2 + 64;
    }
    for (int k = 0; k < 6; ++k) {
      n->Fh[k] = reinterpret_cast<uint16_t*>(p);
      p += sz.n[k] + 64;
    }
    n->Fexp = reinterpret_cast<int*>(p);
    p += 64;
    for (int k = 0; k < 2; ++k) {
      n->Fhp[k] = reinterpret_cast<uint16_t*>(p);
      p += sz.n[4 + k] + 64;
    }
  }
  *out = net.release();
  return INF_OK;
}

int inf_net_destroy(InfNet* n) {
  free_net(n);
  return INF_OK;
}

int inf_net_set_mfma(InfNet* n, int mode) {
  if (!n || (mode != INF_MFMA_F32 && mode != INF_MFMA_BF16X6 && mode != INF_MFMA_F16X3)) return INF_ERR_INVALID;
  // the cached f(0) (ensure_f0) carries the bits of the arithmetic it was computed with
  if (n->mfma_mode != mode) n->f0_batch = -1;
  n->mfma_mode = mode;
  return INF_OK;
}
int inf_net_get_mfma(const InfNet* n) { return n ? n->mfma_mode : -1; }

int inf_net_set_option(InfNet* n, int option, int value) {
  const NetOption* o = n ? find_option(option) : nullptr;
  if (!o || value < 0 || value > o->hi) return -INF_ERR_INVALID;
  const int prev = n->*o->slot;
  n->*o->slot = value;
  if (prev != value && o->resets_f0) n->f0_batch = -1;
  return prev;
}

int inf_net_get_option(const InfNet* n, int option) {
  const NetOption* o = n ? find_option(option) : nullptr;
  return o ? n->*o->slot : -INF_ERR_INVALID;
}

int inf_net_refresh(InfNet* n, void* stream) {
  if (!n) return INF_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  n->f0_batch = -1;
  for (auto& w : n->L) {
    if (w.zb) INF_HIP(hipMemsetAsync(w.zb, 0, sizeof(float) * w.cout, s));
    const int H = n->fc ? 1 : (w.ks == 1 ? 1 : n->H), Wd = n->fc ? 1 : (w.ks == 1 ? 1 : n->W);
    INF_TRY(launch_sigma(w.W, w.u, w.v, w.cout, w.cin, w.ks, H, Wd, w.coeff, w.factor,
                         reinterpret_cast<float*>(n->scratch), s));
    INF_TRY(launch_pack(w.W, w.factor, w.f.A, w.cout, w.cin, w.ks, w.f.Mpad, w.f.Kpad, w.f.pack, s));
    INF_TRY(launch_pack(w.W, w.factor, w.g.A, w.cout, w.cin, w.ks, w.g.Mpad, w.g.Kpad, w.g.pack, s));
  }
  if (n->fch) {
    const int L = (int)n->L.size();
    for (int l = 0; l < L; ++l) {
      const WLayer& w = n->L[l];
      const int nrt = l == L - 1 ? 1 : 8, nks = l == 0 ? 1 : 4;
      INF_TRY(launch_fc_split_h3(w.f.A, w.cout, w.f.Kpad, nrt, nks, n->fch + n->fch_off[l], n->fchexp + l, s));
      // transposed position j = L-1-l: rows cin, k = cout (w.g.A = W^T, row stride g.Kpad), position j's tile shape
      const int j = L - 1 - l, trt = j == L - 1 ? 1 : 8, tks = j == 0 ? 1 : 4;
      INF_TRY(launch_fc_split_h3(w.g.A, w.cin, w.g.Kpad, trt, tks, n->fcht + n->fch_off[j], n->fchtexp + j, s));
    }
  }
  if (n->fused) {
    const WLayer &l0 = n->L[0], &l1 = n->L[1], &l2 = n->L[2];
    const int H = n->fhid;
    INF_TRY(launch_pack(l0.W, l0.factor, n->F1f, l0.cout, l0.cin, 3, H, n->K1pad, PK_IM2COL_FWD, s, 1));
    INF_TRY(launch_pack(l2.W, l2.factor, n->F1b, l2.cout, l2.cin, 3, H, n->K1pad, PK_IM2COL_BWD, s, 1));
    INF_TRY(launch_pack(l1.W, l1.factor, n->F2f, H, H, 1, H, H, PK_ROWMAJOR, s, 1));
    INF_TRY(launch_pack(l1.W, l1.factor, n->F2b, H, H, 1, H, H, PK_TRANSPOSE, s, 1));
    INF_TRY(launch_pack(l2.W, l2.factor, n->F3f, l2.cout, l2.cin, 3, n->M3pad, H, PK_TAPS_FWD, s, 1));
    INF_TRY(launch_pack(l0.W, l0.factor, n->F3b, l0.cout, l0.cin, 3, n->M3pad, H, PK_TAPS_BWD, s, 1));
    const float* src[6] = {n->F1f, n->F1b, n->F2f, n->F2b, n->F3f, n->F3b};
    const FusedSizes cnt(n);
    for (int i = 0; i < 6; ++i) INF_TRY(launch_split3(src[i], n->Fs[i], (long)cnt.n[i], s));
    for (int i = 0; i < 6; ++i)
      INF_TRY(launch_split2h(src[i], n->Fh[i], (long)cnt.n[i], n->Fexp + 3 * (i & 1) + i / 2, s));
    for (int i = 0; i < 2; ++i) INF_TRY(launch_permute_k23(n->Fh[4 + i], n->Fhp[i], (long)cnt.n[4 + i] / 512, s));
  }
  return INF_OK;
}

}  // extern "C"
