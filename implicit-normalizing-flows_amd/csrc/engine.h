// What the host-side translation units of libinflow share: the net plan, the carved workspace views and the functions
// that cross files.  Everything else in those files is file-local.
//
//   engine_plan.hip    net plans, per-net options, workspace carving
//   engine_chain.hip   the forward / VJP launch chains and the boundary-layout helpers
//   engine_solve.hip   readback slots, the Broyden drivers, the Banach fallback, the fc block driver, the root-find entries
//   engine_logdet.hip  the fused series, the eval schedules, the log-det estimators
//   engine_grad.hip    the parameter-gradient chains
//   engine.hip         last-error and profiling state, shutdown, flow glue, debug entries
#pragma once
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <functional>
#include <vector>

#include "glue.h"
#include "kernels.h"

// Events the engine records between its own launches (the host's Broyden readbacks, the side-stream fork / join, the
// profiling brackets) skip the system-scope fence: a system-scope release writes back and invalidates the caches, so the
// next kernel starts with a cold L2 and the CP idles ≈ 5 µs per event (kernel trace).  What the host
// reads through these events lives in coherent pinned memory written by the kernels / copies themselves.
constexpr unsigned INF_EV_SYNC = hipEventDisableTiming | hipEventDisableSystemFence;
constexpr unsigned INF_EV_TIMING = hipEventDisableSystemFence;

namespace inf {

constexpr int TAPS_MAX_CH = 64;   // 3x3 convs with fewer output channels than this use packed taps
constexpr int SERIES_MAX = 128;

struct Operand {
  int load = BL_DIRECT;  // B-operand loader
  int taps = 0;          // output is packed taps (3x3, small M) -> conv_out sums 9 shifts
  int M = 0, Mpad = 0, K = 0, Kpad = 0;
  int pack = PK_ROWMAJOR;
  float* A = nullptr;
};

struct WLayer {
  int kind = 0, cin = 0, cout = 0, ks = 1;
  const float *W = nullptr, *b = nullptr, *u = nullptr, *v = nullptr;
  float coeff = 1.f;
  int act = ACT_NONE;             // activation applied to this layer's output
  const float* act_beta = nullptr;
  Operand f, g;                   // forward, vjp
  float* factor = nullptr;        // device [factor, sigma]
  float* zb = nullptr;            // bias-free layer: the engine's zero vector (cout floats in InfNet::dev) that b points at
};

}  // namespace inf

struct InfNet {
  int C = 0, H = 1, W = 1, P = 1, d = 0;
  bool fc = false;
  int pre_act = inf::ACT_NONE;
  const float* pre_beta = nullptr;
  std::vector<inf::WLayer> L;
  int hidden_max = 0;      // channels of the widest intermediate activation
  int rows_max = 0;        // rows of the widest output-stage buffer Y
  float* dev = nullptr;    // packed operands + factors (owned)
  double* scratch = nullptr;
  size_t scratch_doubles = 0;
  int device = 0;
  // fused 3-1-3 path (fused313.hip): fragment-major operands for forward (f) and VJP (b)
  bool fused = false;
  int fhid = 0, K1pad = 0, M3 = 0, M3pad = 0;
  // fused nets: the tile geometry's per-image maxima over the variants a launch may pick (net313_max_tiles,
  // net313_tile_pixels): tiles, and pixel columns of the tile-indexed d1 / d2 (P on an exact shape, more on a ragged one)
  int ftiles = 0, fpix = 0;
  float *F1f = nullptr, *F1b = nullptr, *F2f = nullptr, *F2b = nullptr, *F3f = nullptr, *F3b = nullptr;
  // F1f..F3b split into three bf16 planes each (launch_split3), same order as F1f..F3b
  uint16_t* Fs[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  // F1f..F3b as two scaled fp16 planes each (launch_split2h, INF_MFMA_F16X3), same order as Fs; their scale
  // exponents per direction: Fexp[3 * vjp + phase]
  uint16_t* Fh[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  int* Fexp = nullptr;
  // Fh[4], Fh[5] (phase C, forward / VJP) with the k index's bits 2 and 3 swapped per 16-k tile (launch_permute_k23)
  uint16_t* Fhp[2] = {nullptr, nullptr};
  int mfma_mode = INF_MFMA_F32;                 // InfMfmaMode of the fused kernel's phase B
  // f(0) of a conv net (the same image for every sample: zero input, zero padding), cached for the first
  // Broyden residual; computed by a launch of the same batch size (same tile variant -> same bits)
  float* f0 = nullptr;
  int f0_batch = -1;
  // per-net options (inf_net_set_option; defaults from the environment at inf_net_create: engine_plan.hip's table)
  int k128 = 1;            // INF_OPT_FUSED_K128
  int eval_overlap = 1;    // INF_OPT_EVAL_OVERLAP (read on net_x of inf_imblock_eval)
  int convergence = INF_CONV_GLOBAL;   // INF_OPT_CONVERGENCE (read on the solved net)
  int line_search = 0;                 // INF_OPT_LINE_SEARCH (read on the solved net)
  int exact_scale = 0;     // INF_OPT_K128_EXACT_SCALE
  int presplit = 1;        // INF_OPT_FUSED_PRESPLIT
  int fc_block = 1;        // INF_OPT_FC_BLOCK (read on net_z of inf_imblock_eval_exact)
  int fc_series = 1;       // INF_OPT_FC_SERIES (read on the first net of inf_logdet_series[_pair])
  int fc_skinny = 1;       // INF_OPT_FC_SKINNY (fc nets over more than FC_NARROW_MAX features: layer_gemm)
  int series_group = 0;    // INF_OPT_SERIES_GROUP (read on the first net of a fused series: 0 the rule, else samples per group)
  // fused fc path (fcnet.hip): the whole net in one launch per evaluation (forward and forward-mode Jacobian)
  bool fcfused = false;
  // f16x3 planes of the fused fc layers (fcnet_h3.hip, filled at refresh): layer l at fch + fch_off[l], exponent fchexp[l]
  uint16_t* fch = nullptr;
  int* fchexp = nullptr;
  std::vector<size_t> fch_off;
  // the transposed layers' planes (fcseries_kernel): position j = W_{L-1-j}^T (w.g.A), the same tile shapes as fch's
  // layer j, at fch_off[j], exponent fchtexp[j]
  uint16_t* fcht = nullptr;
  int* fchtexp = nullptr;
};

namespace inf {

// ---------------------------------------------------------------------------------------------
// workspace views
// ---------------------------------------------------------------------------------------------
struct WS {
  char* base;
  size_t cap, off;
  bool ok = true;
  template <typename T>
  T* take(size_t n) {
    off = (off + 255) & ~(size_t)255;
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += n * sizeof(T);
    if (off > cap) ok = false;
    return p;
  }
};

struct Bufs {
  float *h0, *h1, *Y;
  std::vector<float*> D;   // saved activation derivatives, one per hidden layer
  float *xin, *xemb, *fx, *xa, *xb, *ga, *gb, *upd, *dx, *dg, *lowest, *va, *vb, *eps_t, *zero, *tmp;
  float *fcur, *flow;      // root solve: f(z) of the latest residual evaluation / of the lowest iterate
  float* fspec;            // root solve: f(z) of the speculative iteration in flight (broyden_core)
  float *U, *VT;
  float *ext0, *ext1;
  double *part, *bpart, *sumsq;   // sumsq: B per-sample sums of squares + 1 (per-sample mode: samples iterating)
  // per-sample convergence (INF_CONV_PER_SAMPLE): state machine, flags, lowest iterate and its f
  double* ps_state;
  int *ps_active, *ps_improved;
  float *ps_lowx, *ps_lowf;
  unsigned int* counter;
  int nchunk;              // per-sample partial chunks of conv_out (residual norms, unfused series)
  float* Y2;               // fused nets: second taps buffer (series terms alternate Y / Y2)
  int snchunk;             // per-sample partial stride of the series slabs (>= tiles per image)
  // fc nets: the device-resident block kernel's (fcblock.hip) exchange words and results: [error word, granules]
  // (zeroed per launch) and [stats, per-sample nstep, lowest_step, prot_break, lowest objective]
  unsigned* bk_sync;
  size_t bk_sync_bytes;
  char* bk_out;
  size_t bk_out_bytes;
  // fc root solve, global rule (broyden_core zero-copy readback): the slot's event, bound by the residual launch itself
  // (OutArgs::stop_ev) when its launcher can, which sets stop_bound; enqueue_sumsq then records no marker after it
  hipEvent_t stop_ev = nullptr;
  bool stop_bound = false;
  // wide fc nets: the split-K partials of launch_gemm_skinny (written and read within one layer's two launches)
  float* kslab = nullptr;
  size_t kslab_bytes = 0;
  bool sample_sums = false;   // conv residuals write each sample's total into bf.part (the readback slot; broyden_core)
};

struct GradBufs {
  std::vector<float*> H, Hd, Ad;     // pre-activations, their tangents, activation tangents (Ad[0]: input)
  std::vector<float*> A;             // layer inputs after their activation (A[0] = preact(x)), computed once per call
  float *gA, *gB, *hA, *hB, *gad, *ga, *Y, *slab, *dWe, *dWe2, *dsig, *xin, *tmp_in, *act;
  float *x_t, *w_t, *e_t, *gx_t;     // fc nets: the internal-layout (d, N) copies of the boundary inputs / x-gradient
  double *bpart, *dot;
  int max_split;
  float* kslab;          // wide fc nets: launch_gemm_skinny's split-K partials (Bufs::kslab)
  size_t kslab_bytes;
};

// ---------------------------------------------------------------------------------------------
// engine_plan.hip
// ---------------------------------------------------------------------------------------------
// Carves the workspace; returns the bytes required (fits iff result <= cap).  With ws == nullptr it only measures.
size_t carve(const InfNet* n, int B, int T, void* ws, size_t cap, Bufs& b);
size_t ws_need(const InfNet* n, int B, int T);
// carve, or INF_ERR_WORKSPACE when there is no workspace or it is too small
inline int carve_ws(const InfNet* n, int B, int T, void* ws, size_t ws_bytes, Bufs& b) {
  return (!ws || carve(n, B, T, ws, ws_bytes, b) > ws_bytes) ? INF_ERR_WORKSPACE : INF_OK;
}

inline bool same_shape(const InfNet* a, const InfNet* b) {
  return a->C == b->C && a->H == b->H && a->W == b->W && a->fc == b->fc && a->d == b->d;
}
// Two fused 3-1-3 nets that one pair launch can run: the same hidden width, and both Swish or both of the other fused
// activations -- the launch picks its instantiation (Swish epilogues reading beta1 / beta2, or the kind switch reading
// Net313Args::act) once, from the first net.  Sin / ELU / Softplus / ReLU mix freely: the kind is a per-net field.
inline bool fused_pair(const InfNet* a, const InfNet* b) {
  return a->fused && b->fused && a->fhid == b->fhid && (a->L[0].act == ACT_SWISH) == (b->L[0].act == ACT_SWISH);
}

// ---------------------------------------------------------------------------------------------
// engine_chain.hip
// ---------------------------------------------------------------------------------------------
GemmArgs gemm_base(const InfNet* n, const Operand& op, const float* X, int in_ch, int B);
void set_out(const InfNet* n, GemmArgs& g, float* out, int out_rows);
int layer_gemm(const InfNet* n, const GemmArgs& g, int load, int epi, float* kslab, size_t kslab_bytes, hipStream_t s);
Net313Args net313_args(const InfNet* n, const float* in, int B, Bufs& bf, bool vjp);
FcArgs fc_args(const InfNet* n, const float* x, int B);
// The output stage over the rows Y that the GEMM (or fused launch) of operand op wrote: a, filled by the caller with
// the mode's inputs and outputs, gets Y, the geometry and the mode, and goes to conv_out / fc_out.
int out_stage(const InfNet* n, const Operand& op, int mode, OutArgs a, float* Y, int B, hipStream_t s);
// the operand whose rows a fused 3-1-3 launch leaves in Y (forward and VJP alike: 9 C packed taps)
inline Operand fused_taps(const InfNet* n) {
  Operand op;
  op.taps = 1;
  op.M = n->M3;
  return op;
}
int run_forward(InfNet* n, const float* x, int B, Bufs& bf, int mode, const OutArgs* oa, hipStream_t s);
int run_vjp(InfNet* n, const float* v, float* vout, const float* xin, const float* eps, double* partial, int B,
            Bufs& bf, hipStream_t s);
// x (boundary layout) -> *xi in the internal layout: x itself, or (fc nets) its transpose in buf
int to_internal(InfNet* n, const float* x, float* buf, int B, hipStream_t s, const float** xi);
int to_boundary(InfNet* n, const float* xi, float* out, int B, hipStream_t s);
// A result bound for `out` in the boundary layout: produce(o) writes it in the internal layout into o, which is out
// itself for a conv net and bf.tmp, transposed into out afterwards, for an fc net.
template <typename Produce>
int write_boundary(InfNet* n, Bufs& bf, float* out, int B, hipStream_t s, Produce&& produce) {
  INF_TRY(produce(n->fc ? bf.tmp : out));
  return n->fc ? to_boundary(n, bf.tmp, out, B, s) : INF_OK;
}

// ---------------------------------------------------------------------------------------------
// engine_solve.hip
// ---------------------------------------------------------------------------------------------
int host_wait(hipEvent_t ev);
// A zeroed stats struct carrying the caller's optional per-sample host arrays.
InfBroydenStats stats_for(const InfBroydenStats* caller);
// Work that follows the solve, queued speculatively when the loop queues no further iteration (the pending one is predicted
// to be the last, or the threshold ends the loop): fn(x, f) runs on the pending iterate and its f; x / f record what it
// was queued for, so the caller can tell whether the solve's result (bf.lowest, bf.flow) is that iterate
struct SpecTail {
  std::function<int(const float* x, const float* f)> fn;
  const float* x = nullptr;
  const float* f = nullptr;
};
// Broyden root of g(z) = xemb - f(z) - z on carved buffers (bf.xemb set); result in bf.lowest, its f in bf.flow; the
// Banach fallback from y after a protective break
int broyden_solve(InfNet* f, const float* y, int B, int T, double eps_in, InfBroydenStats* st, float* diff_detail,
                  Bufs& bf, hipStream_t s, SpecTail* tail = nullptr);
int fc_block_eval(InfNet* nx, InfNet* nz, const float* x, float* z, float* logdet_x, float* logdet_z, int B, int T,
                  double eps_in, InfBroydenStats* stats, Bufs& bf, hipStream_t s);
// releases the calling thread's readback slots and the block kernel's statistics buffer (inf_shutdown)
void solve_release_thread();

// ---------------------------------------------------------------------------------------------
// engine_logdet.hip
// ---------------------------------------------------------------------------------------------
int fc_jacobian(InfNet* n, const float* x, int B, Bufs& bf, const float** tang, hipStream_t s);
// releases the calling thread's side streams (inf_shutdown)
void logdet_release_thread();

}  // namespace inf
