// The output stage of a net and the residual builders of the two Broyden solves: the conv nets' tap sum with its fused
// epilogues, the fc nets' epilogues (narrow: one thread per sample; wide: feature chunks), the first residual of the root
// solve from the cached f(0) with or without the solver's first step, the implicit backward's residual, and the
// per-sample reduction of the chunk partials.  Maps implicit_block.py:60,72 (x_embed and g), :227 (the recompute),
// :186-190 (the backward's g), :422-423 (v.eps) and broyden.py:136-144 (the start at 0).  The per-element arithmetic is
// pointwise_ops.h's.  All kernels are coalesced over the contiguous per-sample dimension and reduce per sample with wave
// shuffles + one LDS stage; cross-block sums go through fixed-order fp64 partial slabs (deterministic, no float atomics).
#include <cstring>

#include "pointwise_ops.h"

namespace inf {

int out_nchunk(int per_sample) { return (per_sample + OUT_CH - 1) / OUT_CH; }
// the wide fc output stage (below); mode: an OutMode or OM_WIDE_VJPRES
static int launch_fc_out_wide(const OutArgs& a, int batch, int mode, int bcast, hipStream_t s);

template <typename F>
static const void* kernel_ptr(F* f) { return reinterpret_cast<const void*>(f); }
// the NCH = 1..SS_MAXCH instantiation of a one-block-per-sample kernel for a sample of nch chunks (null: none)
static const void* pick_nch(const void* const (&table)[SS_MAXCH], int nch) {
  return nch >= 1 && nch <= SS_MAXCH ? table[nch - 1] : nullptr;
}
// A launch that completes a readback event: with stop_ev (and not while profiling) the launch itself completes it
// (hipExtLaunchKernel's stop event: no marker packet after it) and *stop_bound, where given, is set; else a plain launch,
// profiled under `tag` with its algorithmic `bytes`.
static int launch_with_stop_event(const void* fn, dim3 grid, dim3 block, void** args, hipStream_t s, hipEvent_t stop_ev,
                                  bool* stop_bound, int tag, double bytes) {
  const bool prof = prof_enabled();
  if (stop_ev && !prof) {
    INF_HIP(hipExtLaunchKernel(fn, grid, block, args, 0, s, nullptr, stop_ev, 0));
    if (stop_bound) *stop_bound = true;
    return INF_OK;
  }
  if (prof) prof_begin_launch(s);
  INF_HIP(hipLaunchKernel(fn, grid, block, args, 0, s));
  if (prof) prof_end_launch(s, tag, 0.0, bytes);
  return INF_OK;
}

// ------------------------------------------------------------------------------------------
// conv net output stage.  Y holds packed taps Y[b][c*9+t][p] (KS = 3) or rows Y[b][c][p] (KS = 1).
//   s = sum_t Y[b][c*9+t][p + (dy-1, dx-1)]           (zero padding outside the image)
// then (implicit_block.py:60,72,227,422-423; pointwise_ops.h out_epilogue):
//   OM_PLAIN : out0 = s + bias
//   OM_EMBED : out0 = a = s + bias (= nnet_x(x));  out1 = a + x   (x_embed)
//   OM_RESID : out0 = g = (x_embed - a) - z;  out1 = g - g_prev;  [out2 = a];  partial += g^2
//   OM_RECOMP: out0 = (fx - a) + x
//   OM_VJP   : out0 = v = s (* swish'(x_in) for preact nets);  partial += v * eps
// ------------------------------------------------------------------------------------------
// The 9-tap sum at (c, p): every tap loaded from a clamped address (all nine in flight), the out-of-image ones then
// added as +0 -- the same sum as adding only the in-image taps in tap order (s starts at +0 and never becomes -0, so
// s + 0 == s): a bounds-checked load per tap made each thread wait nine times for memory
__device__ __forceinline__ float tap_sum9(const float* yc, int P, int H, int W, int p) {
  const int y = p / W, x = p - y * W;
  float v[9];
  bool ok[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
    ok[t] = yy >= 0 && yy < H && xx >= 0 && xx < W;
    const int yc_ = min(max(yy, 0), H - 1), xc_ = min(max(xx, 0), W - 1);
    v[t] = yc[(long)t * P + yc_ * W + xc_];
  }
  float s = 0.f;
#pragma unroll
  for (int t = 0; t < 9; ++t) s += ok[t] ? v[t] : 0.f;
  return s;
}

template <int KS>
__global__ __launch_bounds__(OUT_CH) void conv_out_kernel(OutArgs a) {
  __shared__ double red[16];
  const int b = blockIdx.y, chunk = blockIdx.x;
  const int P = a.H * a.W, per = a.C * P;
  const long ybase = (long)b * a.y_sample, ebase = (long)b * per;
  const float sp = a.pre_beta ? softplus_f(ldc(a.pre_beta)) : 0.f;
  const int lo = chunk * OUT_CH, hi = min(per, lo + OUT_CH);
  double acc = 0.0;
  for (int i = lo + threadIdx.x; i < hi; i += blockDim.x) {
    const int c = i / P, p = i - c * P;
    float s;
    if constexpr (KS == 1) {
      s = a.Y[ybase + (long)c * P + p];
    } else {
      s = tap_sum9(a.Y + ybase + (long)c * 9 * P, P, a.H, a.W, p);
    }
    out_epilogue(a, a.mode, s, c, ebase + i, sp, acc);
  }
  if (a.partial) {
    const double t = block_sum(acc, red);
    if (threadIdx.x == 0) a.partial[(long)b * a.nchunk + chunk] = t;
  }
}

// OM_RESID with the per-sample total (OutArgs::sample_sums, at most SS_MAXCH chunks per sample): one block per sample, its
// threads each taking one element of every chunk (all loads of the sample issued before the sums), the chunk sums formed
// as conv_out_kernel's blocks form them and added in chunk order (sample_total); partial[b] is the sample's total (the
// pinned readback slot in broyden_core).
template <int KS, int NCH>
__global__ __launch_bounds__(OUT_CH) void conv_out_resid_sample_kernel(OutArgs a) {
  __shared__ double red[16];
  const int b = blockIdx.x;
  const int P = a.H * a.W, per = a.C * P;
  const long ybase = (long)b * a.y_sample, ebase = (long)b * per;
  // every chunk's loads first (the element index clamped into the sample; out-of-sample elements are not stored and
  // add nothing), then the epilogues
  double acc[NCH];
  float sv[NCH], i0v[NCH], i1v[NCH], i2v[NCH];
#pragma unroll
  for (int cc = 0; cc < NCH; ++cc) {
    const int i = min(cc * OUT_CH + (int)threadIdx.x, per - 1);
    const int c = i / P, p = i - c * P;
    if constexpr (KS == 1) sv[cc] = a.Y[ybase + (long)c * P + p];
    else sv[cc] = tap_sum9(a.Y + ybase + (long)c * 9 * P, P, a.H, a.W, p);
    const long ei = ebase + i;
    i0v[cc] = a.in0[ei];
    i1v[cc] = a.in1[ei];
    i2v[cc] = a.in2 ? a.in2[ei] : 0.f;
  }
#pragma unroll
  for (int cc = 0; cc < NCH; ++cc) {
    acc[cc] = 0.0;
    const int i = cc * OUT_CH + threadIdx.x;
    if (i >= per) continue;
    const int c = i / P;
    const long ei = ebase + i;
    const float v = sv[cc] + a.bias[c];
    const float gx = resid_value(i0v[cc], v, i1v[cc]);
    a.out0[ei] = gx;
    if (a.in2) a.out1[ei] = gx - i2v[cc];
    if (a.out2) a.out2[ei] = v;
    acc[cc] += (double)gx * (double)gx;
  }
  const double tot = sample_total<NCH>(acc, red);
  if (threadIdx.x == 0) a.partial[b] = tot;
}

int launch_conv_out(const OutArgs& a, int batch, hipStream_t s) {
  const int per = a.C * a.H * a.W;
  dim3 grid(out_nchunk(per), batch);
  // bytes: the Y rows read (9 taps or 1) + ~3 per-element vectors in/out
  const double bytes = 4.0 * (double)batch * per * (a.ks == 3 ? 9 : 1) + 12.0 * (double)batch * per;
  const int tag = 900 + a.mode * 10 + a.ks;
  if (a.sample_sums) {
    static const void* const k3[SS_MAXCH] = {
        kernel_ptr(&conv_out_resid_sample_kernel<3, 1>), kernel_ptr(&conv_out_resid_sample_kernel<3, 2>),
        kernel_ptr(&conv_out_resid_sample_kernel<3, 3>), kernel_ptr(&conv_out_resid_sample_kernel<3, 4>)};
    static const void* const k1[SS_MAXCH] = {
        kernel_ptr(&conv_out_resid_sample_kernel<1, 1>), kernel_ptr(&conv_out_resid_sample_kernel<1, 2>),
        kernel_ptr(&conv_out_resid_sample_kernel<1, 3>), kernel_ptr(&conv_out_resid_sample_kernel<1, 4>)};
    if (a.mode != OM_RESID || !a.partial || (a.ks != 3 && a.ks != 1)) return INF_ERR_INVALID;
    const void* fn = pick_nch(a.ks == 3 ? k3 : k1, out_nchunk(per));
    if (!fn) return INF_ERR_INVALID;
    OutArgs ka = a;
    void* args[] = {&ka};
    return launch_with_stop_event(fn, dim3(batch), dim3(OUT_CH), args, s, a.stop_ev, a.stop_bound, tag, bytes);
  }
  if (a.ks == 1)
    INF_PROF_LAUNCH(s, tag, bytes, conv_out_kernel<1>, grid, dim3(OUT_CH), 0, s, a);
  else
    INF_PROF_LAUNCH(s, tag, bytes, conv_out_kernel<3>, grid, dim3(OUT_CH), 0, s, a);
  return INF_OK;
}

// ------------------------------------------------------------------------------------------
// The first Broyden residual from the cached f(0): v = f0[i] for every sample, g = (x_embed - v) - z exactly as
// OM_RESID, fcur = v, the return value g^2 for the per-sample sums.  START: the root solve's start in the same launch
// (broyden.py:136-144 + the first line_search step): z = x0 = 0 is written too, then update = -g0, x1 = x0 + update,
// dx = x1 - x0 -- the memset, the residual, neg_kernel and axpy_step_kernel element for element.
// ------------------------------------------------------------------------------------------
template <bool START>
__device__ __forceinline__ double first_resid(float v, const float* xemb, const float* z, float* x0, float* g,
                                              float* fcur, float* upd, float* x1, float* dx, long e) {
  const float xm = xemb[e], zv = START ? 0.f : z[e];
  const float gx = resid_value(xm, v, zv);
  if (START) x0[e] = zv;
  g[e] = gx;
  fcur[e] = v;
  if (START) {
    const float up = -gx;
    upd[e] = up;
    float xe, d;
    broyden_step(zv, up, xe, d);
    x1[e] = xe;
    dx[e] = d;
  }
  return (double)gx * (double)gx;
}
// conv layout (B, per): grid (nchunk, B), chunk partials
__global__ __launch_bounds__(OUT_CH) void resid_bcast_kernel(const float* f0, const float* xemb, const float* z, float* g,
                                                          float* fcur, double* partial, int per, int nchunk) {
  __shared__ double red[16];
  const int b = blockIdx.y, chunk = blockIdx.x;
  const long base = (long)b * per;
  const int lo = chunk * OUT_CH, hi = min(per, lo + OUT_CH);
  double acc = 0.0;
  for (int i = lo + threadIdx.x; i < hi; i += blockDim.x)
    acc += first_resid<false>(f0[i], xemb, z, nullptr, g, fcur, nullptr, nullptr, nullptr, base + i);
  const double t = block_sum(acc, red);
  if (threadIdx.x == 0) partial[(long)b * nchunk + chunk] = t;
}
// conv layout, one block per sample: the sample's total in partial[b], summed as conv_out_resid_sample_kernel does
template <int NCH, bool START>
__device__ __forceinline__ void first_resid_sample(const float* f0, const float* xemb, const float* z, float* x0,
                                                   float* g, float* fcur, double* partial, float* upd, float* x1,
                                                   float* dx, int per, double* red) {
  const int b = blockIdx.x;
  const long base = (long)b * per;
  double acc[NCH];
#pragma unroll
  for (int cc = 0; cc < NCH; ++cc) {
    acc[cc] = 0.0;
    const int i = cc * OUT_CH + threadIdx.x;
    if (i >= per) continue;
    acc[cc] += first_resid<START>(f0[i], xemb, z, x0, g, fcur, upd, x1, dx, base + i);
  }
  const double tot = sample_total<NCH>(acc, red);
  if (threadIdx.x == 0) partial[b] = tot;
}
template <int NCH>
__global__ __launch_bounds__(OUT_CH) void resid_bcast_sample_kernel(const float* f0, const float* xemb, const float* z,
                                                                 float* g, float* fcur, double* partial, int per) {
  __shared__ double red[16];
  first_resid_sample<NCH, false>(f0, xemb, z, nullptr, g, fcur, partial, nullptr, nullptr, nullptr, per, red);
}
template <int NCH>
__global__ __launch_bounds__(OUT_CH) void broyden_start_sample_kernel(const float* f0, const float* xemb, float* x0,
                                                                   float* g, float* fcur, double* partial, float* upd,
                                                                   float* x1, float* dx, int per) {
  __shared__ double red[16];
  first_resid_sample<NCH, true>(f0, xemb, nullptr, x0, g, fcur, partial, upd, x1, dx, per, red);
}
int launch_broyden_start_sample(const float* f0, const float* xemb, float* x0, float* g, float* fcur, double* partial,
                                hipEvent_t stop_ev, bool* stop_bound, float* upd, float* x1, float* dx, int batch,
                                int per, hipStream_t s) {
  static const void* const k[SS_MAXCH] = {
      kernel_ptr(&broyden_start_sample_kernel<1>), kernel_ptr(&broyden_start_sample_kernel<2>),
      kernel_ptr(&broyden_start_sample_kernel<3>), kernel_ptr(&broyden_start_sample_kernel<4>)};
  const void* fn = pick_nch(k, out_nchunk(per));
  if (!fn) return INF_ERR_INVALID;
  void* args[] = {&f0, &xemb, &x0, &g, &fcur, &partial, &upd, &x1, &dx, &per};
  return launch_with_stop_event(fn, dim3(batch), dim3(OUT_CH), args, s, stop_ev, stop_bound, 708,
                                28.0 * batch * per + 4.0 * per);
}

int launch_resid_bcast(const float* f0, const float* xemb, const float* z, float* g, float* fcur, double* partial,
                       int batch, int per, int nchunk, hipStream_t s, int sample_sums, hipEvent_t stop_ev,
                       bool* stop_bound) {
  if (sample_sums) {
    static const void* const k[SS_MAXCH] = {
        kernel_ptr(&resid_bcast_sample_kernel<1>), kernel_ptr(&resid_bcast_sample_kernel<2>),
        kernel_ptr(&resid_bcast_sample_kernel<3>), kernel_ptr(&resid_bcast_sample_kernel<4>)};
    const void* fn = pick_nch(k, out_nchunk(per));
    if (!fn) return INF_ERR_INVALID;
    void* args[] = {&f0, &xemb, &z, &g, &fcur, &partial, &per};
    return launch_with_stop_event(fn, dim3(batch), dim3(OUT_CH), args, s, stop_ev, stop_bound, 709,
                                  16.0 * batch * per + 4.0 * per);
  }
  INF_PROF_LAUNCH(s, 700, 16.0 * batch * per + 4.0 * per, resid_bcast_kernel, dim3(out_nchunk(per), batch),
                  dim3(OUT_CH), 0, s, f0, xemb, z, g, fcur, partial, per, nchunk);
  return INF_OK;
}

// fc layout (d, B) of the same: one thread per sample, the sums in fc_out's / fcnet's order (bit-identical to a
// residual evaluated at z with f(z) = f0)
template <bool START>
__device__ __forceinline__ void first_resid_fc(const float* f0, const float* xemb, const float* z, float* x0, float* g,
                                               float* fcur, double* partial, float* upd, float* x1, float* dx,
                                               int batch, int d) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  double acc = 0.0;
  for (int i = 0; i < d; ++i)
    acc += first_resid<START>(f0[i], xemb, z, x0, g, fcur, upd, x1, dx, (long)i * batch + b);
  partial[b] = acc;
}
__global__ __launch_bounds__(256) void resid_bcast_fc_kernel(const float* f0, const float* xemb, const float* z, float* g,
                                                             float* fcur, double* partial, int batch, int d) {
  first_resid_fc<false>(f0, xemb, z, nullptr, g, fcur, partial, nullptr, nullptr, nullptr, batch, d);
}
__global__ __launch_bounds__(256) void broyden_start_fc_kernel(const float* f0, const float* xemb, float* x0, float* g,
                                                               float* fcur, double* partial, float* upd, float* x1,
                                                               float* dx, int batch, int d) {
  first_resid_fc<true>(f0, xemb, nullptr, x0, g, fcur, partial, upd, x1, dx, batch, d);
}
int launch_broyden_start_fc(const float* f0, const float* xemb, float* x0, float* g, float* fcur, double* partial,
                            hipEvent_t stop_ev, bool* stop_bound, float* upd, float* x1, float* dx, int batch, int d,
                            hipStream_t s) {
  void* args[] = {&f0, &xemb, &x0, &g, &fcur, &partial, &upd, &x1, &dx, &batch, &d};
  return launch_with_stop_event(kernel_ptr(&broyden_start_fc_kernel), dim3((batch + 255) / 256), dim3(256), args, s,
                                stop_ev, stop_bound, 702, 28.0 * batch * d + 8.0 * batch);
}
int launch_resid_bcast_fc(const float* f0, const float* xemb, const float* z, float* g, float* fcur, double* partial,
                          int batch, int d, hipStream_t s) {
  if (d > FC_NARROW_MAX) {                     // wide nets: fc_out_wide's OM_RESID with Y = f0 broadcast, chunk partials
    OutArgs a;
    memset(&a, 0, sizeof(a));
    a.Y = f0;
    a.C = d;
    a.in0 = xemb;
    a.in1 = z;
    a.out0 = g;
    a.out2 = fcur;
    a.partial = partial;
    a.nchunk = out_nchunk(d);
    return launch_fc_out_wide(a, batch, OM_RESID, 1, s);
  }
  INF_PROF_LAUNCH(s, 701, 16.0 * batch * d + 8.0 * batch, resid_bcast_fc_kernel, dim3((batch + 255) / 256),
                  dim3(256), 0, s, f0, xemb, z, g, fcur, partial, batch, d);
  return INF_OK;
}

// Implicit-backward residual (implicit_block.py:186-190): g = (y + v) - grad with v = y^T J (the VJP),
// dg = g - gprev (gprev may be null), per-sample partial sums of g^2.
// Conv layout (B, d): grid (nchunk, B), partial[b * nchunk + chunk].  fc layout (d, B): one thread per
// sample, partial[b].
__device__ __forceinline__ double vjp_resid_elem(const float* v, const float* y, const float* grad, const float* gprev,
                                                 float* g, float* dg, long e) {
  const float gv = vjp_resid_value(y[e], v[e], grad[e]);
  g[e] = gv;
  if (gprev) dg[e] = gv - gprev[e];
  return (double)gv * (double)gv;
}
__global__ __launch_bounds__(256) void vjp_resid_kernel(const float* v, const float* y, const float* grad,
                                                        const float* gprev, float* g, float* dg, double* partial,
                                                        int d, int nchunk) {
  __shared__ double red[16];
  const int b = blockIdx.y, chunk = blockIdx.x;
  const long base = (long)b * d;
  const int lo = chunk * OUT_CH, hi = min(d, lo + OUT_CH);
  double acc = 0.0;
  for (int i = lo + threadIdx.x; i < hi; i += blockDim.x) acc += vjp_resid_elem(v, y, grad, gprev, g, dg, base + i);
  const double t = block_sum(acc, red);
  if (threadIdx.x == 0) partial[(long)b * nchunk + chunk] = t;
}
__global__ void vjp_resid_fc_kernel(const float* v, const float* y, const float* grad, const float* gprev, float* g,
                                    float* dg, double* partial, int d, int batch) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  double acc = 0.0;
  for (int j = 0; j < d; ++j) acc += vjp_resid_elem(v, y, grad, gprev, g, dg, (long)j * batch + b);
  partial[b] = acc;
}
int launch_vjp_resid(const float* v, const float* y, const float* grad, const float* gprev, float* g, float* dg,
                     double* partial, int batch, int d, int nchunk, int fc, hipStream_t s) {
  if (fc && d > FC_NARROW_MAX) {               // wide fc nets: partial[b * nchunk + chunk]
    OutArgs a;
    memset(&a, 0, sizeof(a));
    a.Y = v;
    a.C = d;
    a.in0 = y;
    a.in1 = grad;
    a.in2 = gprev;
    a.out0 = g;
    a.out1 = dg;
    a.partial = partial;
    a.nchunk = nchunk;
    return launch_fc_out_wide(a, batch, OM_WIDE_VJPRES, 0, s);
  }
  if (fc) {
    hipLaunchKernelGGL(vjp_resid_fc_kernel, dim3((batch + 255) / 256), dim3(256), 0, s, v, y, grad, gprev, g, dg,
                       partial, d, batch);
  } else {
    hipLaunchKernelGGL(vjp_resid_kernel, dim3(out_nchunk(d), batch), dim3(256), 0, s, v, y, grad, gprev, g, dg,
                       partial, d, nchunk);
  }
  INF_CHECK_LAUNCH();
  return INF_OK;
}

// fc nets: tensors are feature-major (d, B); Y rows are (d, B); one thread per sample.
__global__ __launch_bounds__(256) void fc_out_kernel(OutArgs a, int batch) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  const float sp = a.pre_beta ? softplus_f(*a.pre_beta) : 0.f;
  double acc = 0.0;
  for (int c = 0; c < a.C; ++c) {
    const long ei = (long)c * batch + b;
    out_epilogue(a, a.mode, a.Y[ei], c, ei, sp, acc);
  }
  if (a.partial) a.partial[b] = acc;
}

// Wide fc nets (d > FC_NARROW_MAX): the same epilogues on a grid of (feature chunk of OUT_CH rows, sample block of
// 2^lsb columns).  A thread owns one sample column of its block and every (OUT_CH >> lsb)-th feature row of the chunk,
// so a wave's loads run along the contiguous batch index of the (d, B) layout (and over consecutive rows when the
// block is narrower than a wave).  The per-sample fp64 partial of a chunk: each thread's rows in row order, then a
// fixed LDS tree over the threads of the column; partial[b * nchunk + chunk], summed in chunk order by
// reduce_partials_kernel / series_combine_kernel -- nothing depends on scheduling.
//   bcast: Y holds d values (the cached f(0), bias included) broadcast over the batch (resid_bcast_fc's residual)
//   OM_WIDE_VJPRES (internal): the implicit backward's residual, g = (in0 + Y) - in1 with Y = y^T J, in0 = y, in1 = grad
template <int MODE>
__global__ __launch_bounds__(OUT_CH) void fc_out_wide_kernel(OutArgs a, int batch, int lsb, int bcast) {
  __shared__ double red[OUT_CH];
  const int sbw = 1 << lsb;
  const int chunk = blockIdx.x, tid = threadIdx.x;
  const int b = blockIdx.y * sbw + (tid & (sbw - 1));
  const int lo = chunk * OUT_CH, hi = min(a.C, lo + OUT_CH), rstep = OUT_CH >> lsb;
  const float sp = (MODE == OM_VJP && a.pre_beta) ? softplus_f(ldc(a.pre_beta)) : 0.f;
  double acc = 0.0;
  if (b < batch) {
#pragma unroll 4
    for (int c = lo + (tid >> lsb); c < hi; c += rstep) {
      const long ei = (long)c * batch + b;
      out_epilogue<true>(a, MODE, bcast ? a.Y[c] : a.Y[ei], c, ei, sp, acc);
    }
  }
  if constexpr (MODE == OM_RESID || MODE == OM_VJP || MODE == OM_WIDE_VJPRES) {
    if (!a.partial) return;                      // (uniform over the block)
    red[tid] = acc;
    __syncthreads();
    for (int st = OUT_CH / 2; st >= sbw; st >>= 1) {
      if (tid < st) red[tid] += red[tid + st];
      __syncthreads();
    }
    if (tid < sbw && b < batch) a.partial[(long)b * a.nchunk + chunk] = red[tid];
  }
}

static int launch_fc_out_wide(const OutArgs& a, int batch, int mode, int bcast, hipStream_t s) {
  const int nch = out_nchunk(a.C);
  if (a.partial && a.nchunk != nch) return INF_ERR_INVALID;
  if ((mode == OM_RESID || mode == OM_WIDE_VJPRES) && !a.partial) return INF_ERR_INVALID;
  int lsb = 0;
  while (lsb < 6 && (1 << lsb) < batch) ++lsb;   // sample block: the batch rounded up to a power of two, a wave at most
  const dim3 grid(nch, (batch + (1 << lsb) - 1) >> lsb);
  // bytes: Y and ~3 per-element vectors in / out
  const double by = 16.0 * (double)batch * a.C;
#define FCW_K(M_)                                                                                                  \
  case M_:                                                                                                         \
    INF_PROF_LAUNCH(s, 950 + M_, by, fc_out_wide_kernel<M_>, grid, dim3(OUT_CH), 0, s, a, batch, lsb, bcast);       \
    return INF_OK;
  switch (mode) {
    FCW_K(OM_PLAIN) FCW_K(OM_EMBED) FCW_K(OM_RESID) FCW_K(OM_RECOMP) FCW_K(OM_VJP) FCW_K(OM_WIDE_VJPRES)
  }
#undef FCW_K
  return INF_ERR_INVALID;
}

int launch_fc_out(const OutArgs& a, int batch, hipStream_t s) {
  if (a.C > FC_NARROW_MAX) return launch_fc_out_wide(a, batch, a.mode, 0, s);
  hipLaunchKernelGGL(fc_out_kernel, dim3((batch + 255) / 256), dim3(256), 0, s, a, batch);
  INF_CHECK_LAUNCH();
  return INF_OK;
}

// per-sample totals of the chunk partials, in chunk order from 0.0
__global__ void reduce_partials_kernel(const double* partial, int batch, int nchunk, double* out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  double s = 0.0;
  for (int c = 0; c < nchunk; ++c) s += partial[(long)b * nchunk + c];
  out[b] = s;
}
int launch_reduce_partials(const double* partial, int batch, int nchunk, double* out, hipStream_t s, hipEvent_t stop_ev,
                           bool* stop_bound) {
  void* args[] = {&partial, &batch, &nchunk, &out};
  return launch_with_stop_event(kernel_ptr(&reduce_partials_kernel), dim3((batch + 255) / 256), dim3(256), args, s,
                                stop_ev, stop_bound, 705, 8.0 * batch * nchunk + 8.0 * batch);
}

}  // namespace inf
