// Lipschitz power iteration on the engine: compute_weight(update=True) of InducedNormConv2d /
// InducedNormLinear (mixed_lipschitz.py:85-124 linear, :276-326 1x1, :328-386 kxk):
//
//   repeat up to max_iters:  u <- normalize(W v)      (2 -> 2: F.normalize, x / max(|x|_2, 1e-12), in place;
//                            v <- normalize(W^T u)     other induced norms: the forms at PINorm below)
//                            stop when |u - u_old|/sqrt(n_u) < atol + rtol max(u)  and the same for v
//   sigma = u . (W v)  -> scale
//
// W v is conv2d(v.view(1, cin, H, W), W, padding k//2) for a k x k conv, W @ v for 1x1 / linear;
// W^T u is the matching conv_transpose2d / mv(W^T).  The work per iteration is tiny (one image),
// so the kernels are simple: a direct conv with one thread per output element, and one 1024-thread
// workgroup per vector for the norm / in-place update / error / max (fp64 sums).  The stopping test
// is evaluated on the device; a `done` flag turns the remaining kernels of a speculative chunk of
// iterations into no-ops, so the host looks at the flag once per chunk instead of every iteration.
#include <algorithm>
#include <cstring>
#include <vector>

#include "kernels.h"

namespace inf {

struct PIState {
  int done, iters, use_tol, pad;
  float atol, rtol;
  double err_u, max_u;   // of the u update of the current iteration
  double sigma;
};

struct PIOp {
  const float* W;
  int cin, cout, ks, H, Wd;   // conv: spatial dims; 1x1 / linear: H = Wd = 1, ks = 1
};

// y = W x  (x: cin*H*W, y: cout*H*W)
__global__ void pi_apply_w(PIOp op, const float* __restrict__ x, float* __restrict__ y, const PIState* st) {
  if (st && st->done) return;
  const int P = op.H * op.Wd;
  const long n = (long)op.cout * P;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int o = (int)(i / P), p = (int)(i - (long)o * P);
  const int py = p / op.Wd, px = p - py * op.Wd;
  const int ks = op.ks, r = ks / 2, kk = ks * ks;
  const float* w = op.W + (long)o * op.cin * kk;
  float acc = 0.f;
  for (int c = 0; c < op.cin; ++c)
    for (int t = 0; t < kk; ++t) {
      const int yy = py + t / ks - r, xx = px + t % ks - r;
      if (yy >= 0 && yy < op.H && xx >= 0 && xx < op.Wd) acc = fmaf(w[c * kk + t], x[(long)c * P + yy * op.Wd + xx], acc);
    }
  y[i] = acc;
}

// x = W^T y  (conv_transpose2d with the same padding)
__global__ void pi_apply_wt(PIOp op, const float* __restrict__ y, float* __restrict__ x, const PIState* st) {
  if (st && st->done) return;
  const int P = op.H * op.Wd;
  const long n = (long)op.cin * P;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int c = (int)(i / P), q = (int)(i - (long)c * P);
  const int qy = q / op.Wd, qx = q - qy * op.Wd;
  const int ks = op.ks, r = ks / 2, kk = ks * ks;
  float acc = 0.f;
  for (int o = 0; o < op.cout; ++o) {
    const float* w = op.W + ((long)o * op.cin + c) * kk;
    for (int t = 0; t < kk; ++t) {
      const int yy = qy - t / ks + r, xx = qx - t % ks + r;
      if (yy >= 0 && yy < op.H && xx >= 0 && xx < op.Wd) acc = fmaf(w[t], y[(long)o * P + yy * op.Wd + xx], acc);
    }
  }
  x[i] = acc;
}

// Few-output variants (fewer than PI_WAVE_MAX outputs, e.g. the 512 -> 3 conv's W v: 3072 outputs of
// 4608 terms): one wave per output element, the lanes split the reduction (fixed order), wave sum.
constexpr long PI_WAVE_MAX = 65536;
__global__ __launch_bounds__(256) void pi_apply_w_wave(PIOp op, const float* __restrict__ x, float* __restrict__ y,
                                                       const PIState* st) {
  if (st && st->done) return;
  const int P = op.H * op.Wd;
  const long n = (long)op.cout * P;
  const long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (i >= n) return;                               // wave-uniform
  const int o = (int)(i / P), p = (int)(i - (long)o * P);
  const int py = p / op.Wd, px = p - py * op.Wd;
  const int ks = op.ks, r = ks / 2, kk = ks * ks;
  const float* w = op.W + (long)o * op.cin * kk;
  float acc = 0.f;
  for (int j = lane; j < op.cin * kk; j += 64) {
    const int c = j / kk, t = j - c * kk;
    const int yy = py + t / ks - r, xx = px + t % ks - r;
    if (yy >= 0 && yy < op.H && xx >= 0 && xx < op.Wd) acc = fmaf(w[j], x[(long)c * P + yy * op.Wd + xx], acc);
  }
  acc = wave_sum(acc);
  if (lane == 0) y[i] = acc;
}
__global__ __launch_bounds__(256) void pi_apply_wt_wave(PIOp op, const float* __restrict__ y, float* __restrict__ x,
                                                        const PIState* st) {
  if (st && st->done) return;
  const int P = op.H * op.Wd;
  const long n = (long)op.cin * P;
  const long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (i >= n) return;
  const int c = (int)(i / P), q = (int)(i - (long)c * P);
  const int qy = q / op.Wd, qx = q - qy * op.Wd;
  const int ks = op.ks, r = ks / 2, kk = ks * ks;
  float acc = 0.f;
  for (int j = lane; j < op.cout * kk; j += 64) {
    const int o = j / kk, t = j - o * kk;
    const int yy = qy - t / ks + r, xx = qx - t % ks + r;
    if (yy >= 0 && yy < op.H && xx >= 0 && xx < op.Wd)
      acc = fmaf(op.W[((long)o * op.cin + c) * kk + t], y[(long)o * P + yy * op.Wd + xx], acc);
  }
  acc = wave_sum(acc);
  if (lane == 0) x[i] = acc;
}
static void pi_launch_w(const PIOp& op, const float* x, float* y, const PIState* st, hipStream_t s) {
  const long n = (long)op.cout * op.H * op.Wd;
  if (n < PI_WAVE_MAX)
    hipLaunchKernelGGL(pi_apply_w_wave, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, op, x, y, st);
  else
    hipLaunchKernelGGL(pi_apply_w, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, op, x, y, st);
}
static void pi_launch_wt(const PIOp& op, const float* y, float* x, const PIState* st, hipStream_t s) {
  const long n = (long)op.cin * op.H * op.Wd;
  if (n < PI_WAVE_MAX)
    hipLaunchKernelGGL(pi_apply_wt_wave, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, op, y, x, st);
  else
    hipLaunchKernelGGL(pi_apply_wt, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, op, y, x, st);
}

__device__ double block_reduce_sum(double v, double* red) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();
  if (lane == 0) red[wid] = v;
  __syncthreads();
  double s = 0.0;
  for (int k = 0; k < nw; ++k) s += red[k];
  return s;
}
__device__ double block_reduce_max(double v, double* red) {
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();
  if (lane == 0) red[wid] = v;
  __syncthreads();
  double m = red[0];
  for (int k = 1; k < nw; ++k) m = fmax(m, red[k]);
  return m;
}

// One workgroup: vec <- s / max(|s|, 1e-12) in place; err = |vec_new - vec_old| / sqrt(n), max(vec_new).
// which = 0 (u): stash err/max; which = 1 (v): decide convergence, count the iteration.
__global__ __launch_bounds__(1024) void pi_normalize(const float* __restrict__ s, float* vec, long n, PIState* st,
                                                     int which) {
  __shared__ double red[16];
  if (st->done) return;
  double ss = 0.0;
  for (long i = threadIdx.x; i < n; i += blockDim.x) ss += (double)s[i] * (double)s[i];
  ss = block_reduce_sum(ss, red);
  const float nrm = fmaxf((float)sqrt(ss), 1e-12f);
  double e = 0.0, mx = -INFINITY;
  for (long i = threadIdx.x; i < n; i += blockDim.x) {
    const float nv = s[i] / nrm;
    const double d = (double)nv - (double)vec[i];
    e += d * d;
    mx = fmax(mx, (double)nv);
    vec[i] = nv;
  }
  e = block_reduce_sum(e, red);
  mx = block_reduce_max(mx, red);
  if (threadIdx.x != 0) return;
  const double err = sqrt(e) / sqrt((double)n);
  if (which == 0) {
    st->err_u = err;
    st->max_u = mx;
    return;
  }
  st->iters += 1;
  if (st->use_tol) {
    const double tol_u = (double)st->atol + (double)st->rtol * st->max_u;
    const double tol_v = (double)st->atol + (double)st->rtol * mx;
    if (st->err_u < tol_u && err < tol_v) st->done = 1;
  }
}

// Long vectors (a k x k conv's u or v: cout*H*W up to 512K) use PI_NB workgroups instead of one:
//   pi_dot_part   partial sums of a.b per workgroup (grid-stride, fixed order)
//   pi_norm_apply every workgroup re-reduces the partials (same order, same result), normalises its
//                 slice in place and writes partial |new - old|^2 and max
//   pi_norm_final one workgroup: err / max / convergence as pi_normalize
constexpr int PI_NB = 256;
constexpr long PI_MULTI_MIN = 16384;
__global__ __launch_bounds__(256) void pi_dot_part(const float* __restrict__ a, const float* __restrict__ b, long n,
                                                   const PIState* st, double* part) {
  __shared__ double red[16];
  if (st && st->done) return;
  double acc = 0.0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    acc += (double)a[i] * (double)b[i];
  acc = block_reduce_sum(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}
__global__ __launch_bounds__(256) void pi_norm_apply(const float* __restrict__ s, float* vec, long n,
                                                     const PIState* st, const double* part, double* part_e,
                                                     double* part_m) {
  __shared__ double red[16];
  if (st->done) return;
  double ss = threadIdx.x < gridDim.x ? part[threadIdx.x] : 0.0;
  ss = block_reduce_sum(ss, red);
  const float nrm = fmaxf((float)sqrt(ss), 1e-12f);
  double e = 0.0, mx = -INFINITY;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float nv = s[i] / nrm;
    const double d = (double)nv - (double)vec[i];
    e += d * d;
    mx = fmax(mx, (double)nv);
    vec[i] = nv;
  }
  e = block_reduce_sum(e, red);
  mx = block_reduce_max(mx, red);
  if (threadIdx.x == 0) {
    part_e[blockIdx.x] = e;
    part_m[blockIdx.x] = mx;
  }
}
__global__ __launch_bounds__(256) void pi_norm_final(long n, int nparts, PIState* st, const double* part_e,
                                                     const double* part_m, int which) {
  __shared__ double red[16];
  if (st->done) return;
  double e = threadIdx.x < nparts ? part_e[threadIdx.x] : 0.0;
  double mx = threadIdx.x < nparts ? part_m[threadIdx.x] : -INFINITY;
  e = block_reduce_sum(e, red);
  mx = block_reduce_max(mx, red);
  if (threadIdx.x != 0) return;
  const double err = sqrt(e) / sqrt((double)n);
  if (which == 0) {
    st->err_u = err;
    st->max_u = mx;
    return;
  }
  st->iters += 1;
  if (st->use_tol) {
    const double tol_u = (double)st->atol + (double)st->rtol * st->max_u;
    const double tol_v = (double)st->atol + (double)st->rtol * mx;
    if (st->err_u < tol_u && err < tol_v) st->done = 1;
  }
}
__global__ __launch_bounds__(256) void pi_sigma_final(const double* part, int nparts, PIState* st, float* scale) {
  __shared__ double red[16];
  double v = threadIdx.x < nparts ? part[threadIdx.x] : 0.0;
  v = block_reduce_sum(v, red);
  if (threadIdx.x == 0) {
    st->sigma = v;
    if (scale) *scale = (float)v;
  }
}
// ---- induced norms other than 2 -> 2 (mixed_lipschitz.py:406-449).  The normalisation of a vector x depends on
// the norm p of the space it lives in (v: the domain, u: the codomain); besides x / |x|_2 there are two forms:
//   PI_ONEHOT  v with domain 1, u with codomain inf: +1 at the lowest index of max |x|, 0 elsewhere (the
//              reference's projmax_ drops the sign)
//   PI_POWER   s a^e / (sum (a^e)^np)^inv with a = |x| / max |x|, s = sign(x) (+1 at 0);
//              v: e = 1/(p-1), np = p, inv = 1/p;  u: e = q-1, np = q/(q-1), inv = (q-1)/q
//   PI_SIGN    the limits domain = inf / codomain = 1 of PI_POWER: the sign vector, divisor 1
// The powers run in fp32 (powf), the sums in fp64 in a fixed order; err / max / the stopping rule are those of
// pi_normalize.
enum { PI_L2 = 0, PI_ONEHOT = 1, PI_POWER = 2, PI_SIGN = 3 };
struct PINorm {
  int mode;
  float e, np;
  double inv;
};
static PINorm pi_norm_of(float p, bool is_u) {
  PINorm nm = {PI_L2, 0.f, 0.f, 0.0};
  if (p == 0.f || p == 2.f) return nm;
  const bool inf = std::isinf(p);
  if (is_u ? inf : p == 1.f) {
    nm.mode = PI_ONEHOT;
  } else if (is_u ? p == 1.f : inf) {
    nm.mode = PI_SIGN;
  } else {
    nm.mode = PI_POWER;
    const double q = (double)p;
    nm.e = (float)(is_u ? q - 1.0 : 1.0 / (q - 1.0));
    nm.np = (float)(is_u ? q / (q - 1.0) : q);
    nm.inv = is_u ? (q - 1.0) / q : 1.0 / q;
  }
  return nm;
}

// (|x|, index) pairs: the larger |x| wins, ties go to the lower index, so the order of combination does not matter
struct PIAmax {
  float a;
  long long i;
};
__device__ __forceinline__ PIAmax pi_amax_pick(PIAmax x, PIAmax y) {
  return (y.a > x.a || (y.a == x.a && y.i < x.i)) ? y : x;
}
__device__ PIAmax block_reduce_amax(PIAmax v, float* red_a, long long* red_i) {
  for (int o = 32; o > 0; o >>= 1) {
    PIAmax w;
    w.a = __shfl_xor(v.a, o);
    w.i = __shfl_xor(v.i, o);
    v = pi_amax_pick(v, w);
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();
  if (lane == 0) {
    red_a[wid] = v.a;
    red_i[wid] = v.i;
  }
  __syncthreads();
  PIAmax m = {red_a[0], red_i[0]};
  for (int k = 1; k < nw; ++k) m = pi_amax_pick(m, PIAmax{red_a[k], red_i[k]});
  return m;
}
__device__ __forceinline__ float pi_sign(float x) { return x < 0.f ? -1.f : 1.f; }

// err / max of one vector's update and, after v's, the stopping rule (thread 0 only; as pi_normalize's tail)
__device__ void pi_finish(PIState* st, int which, double e, double mx, long n) {
  const double err = sqrt(e) / sqrt((double)n);
  if (which == 0) {
    st->err_u = err;
    st->max_u = mx;
    return;
  }
  st->iters += 1;
  if (st->use_tol) {
    const double tol_u = (double)st->atol + (double)st->rtol * st->max_u;
    const double tol_v = (double)st->atol + (double)st->rtol * mx;
    if (st->err_u < tol_u && err < tol_v) st->done = 1;
  }
}

// One workgroup, any form but PI_L2.  PI_POWER overwrites s with s a^e on the way (s is iteration scratch).
__global__ __launch_bounds__(1024) void pi_normalize_p(float* __restrict__ s, float* vec, long n, PIState* st,
                                                       int which, PINorm nm) {
  __shared__ double red[16];
  __shared__ float red_a[16];
  __shared__ long long red_i[16];
  if (st->done) return;
  PIAmax am = {-1.f, 0x7fffffffffffffffLL};
  if (nm.mode != PI_SIGN) {
    for (long i = threadIdx.x; i < n; i += blockDim.x) {
      const float a = fabsf(s[i]);
      if (a > am.a) am = PIAmax{a, (long long)i};
    }
    am = block_reduce_amax(am, red_a, red_i);
  }
  float nrm = 1.f;
  if (nm.mode == PI_POWER) {
    double ss = 0.0;
    for (long i = threadIdx.x; i < n; i += blockDim.x) {
      const float x = s[i];
      const float t = powf(fabsf(x) / am.a, nm.e);
      ss += (double)powf(t, nm.np);
      s[i] = pi_sign(x) * t;
    }
    ss = block_reduce_sum(ss, red);
    nrm = (float)pow(ss, nm.inv);
  }
  double e = 0.0, mx = -INFINITY;
  for (long i = threadIdx.x; i < n; i += blockDim.x) {
    const float nv = nm.mode == PI_ONEHOT ? (i == am.i ? 1.f : 0.f) : nm.mode == PI_SIGN ? pi_sign(s[i]) : s[i] / nrm;
    const double d = (double)nv - (double)vec[i];
    e += d * d;
    mx = fmax(mx, (double)nv);
    vec[i] = nv;
  }
  e = block_reduce_sum(e, red);
  mx = block_reduce_max(mx, red);
  if (threadIdx.x == 0) pi_finish(st, which, e, mx, n);
}

// The PI_NB-workgroup form for long vectors:
//   pi_amax_part  per-workgroup (max |x|, lowest index of it)            (PI_ONEHOT, PI_POWER)
//   pi_pow_part   every workgroup re-reduces the maxima, overwrites its slice of s with s a^e and writes its
//                 partial sum of (a^e)^np                                   (PI_POWER)
//   pi_apply_p    every workgroup re-reduces the partials of the stage before, writes its slice of the new vector
//                 and its partial |new - old|^2 and max
//   pi_norm_final as for PI_L2
__global__ __launch_bounds__(256) void pi_amax_part(const float* __restrict__ s, long n, const PIState* st,
                                                    double* part_a, double* part_i) {
  __shared__ float red_a[16];
  __shared__ long long red_i[16];
  if (st->done) return;
  PIAmax am = {-1.f, 0x7fffffffffffffffLL};
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float a = fabsf(s[i]);
    if (a > am.a) am = PIAmax{a, (long long)i};
  }
  am = block_reduce_amax(am, red_a, red_i);
  if (threadIdx.x == 0) {
    part_a[blockIdx.x] = (double)am.a;
    part_i[blockIdx.x] = __longlong_as_double(am.i);
  }
}
// the (max, index) over the PI_NB partials (blockDim.x >= PI_NB)
__device__ PIAmax pi_amax_of_parts(const double* part_a, const double* part_i, int nparts, float* red_a,
                                   long long* red_i) {
  PIAmax am = {-1.f, 0x7fffffffffffffffLL};
  if ((int)threadIdx.x < nparts) am = PIAmax{(float)part_a[threadIdx.x], __double_as_longlong(part_i[threadIdx.x])};
  return block_reduce_amax(am, red_a, red_i);
}
__global__ __launch_bounds__(256) void pi_pow_part(float* __restrict__ s, long n, const PIState* st, PINorm nm,
                                                   const double* part_a, const double* part_i, double* part_s) {
  __shared__ double red[16];
  __shared__ float red_a[16];
  __shared__ long long red_i[16];
  if (st->done) return;
  const PIAmax am = pi_amax_of_parts(part_a, part_i, gridDim.x, red_a, red_i);
  double ss = 0.0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float x = s[i];
    const float t = powf(fabsf(x) / am.a, nm.e);
    ss += (double)powf(t, nm.np);
    s[i] = pi_sign(x) * t;
  }
  ss = block_reduce_sum(ss, red);
  if (threadIdx.x == 0) part_s[blockIdx.x] = ss;
}
// in: part_a / part_i (PI_ONEHOT) or part_s (PI_POWER); out: part_e / part_m, which no workgroup reads here
__global__ __launch_bounds__(256) void pi_apply_p(const float* __restrict__ s, float* vec, long n, const PIState* st,
                                                  PINorm nm, const double* part_a, const double* part_i,
                                                  const double* part_s, double* part_e, double* part_m) {
  __shared__ double red[16];
  __shared__ float red_a[16];
  __shared__ long long red_i[16];
  if (st->done) return;
  long long hot = -1;
  float nrm = 1.f;
  if (nm.mode == PI_ONEHOT) {
    hot = pi_amax_of_parts(part_a, part_i, gridDim.x, red_a, red_i).i;
  } else if (nm.mode == PI_POWER) {
    double ss = threadIdx.x < gridDim.x ? part_s[threadIdx.x] : 0.0;
    ss = block_reduce_sum(ss, red);
    nrm = (float)pow(ss, nm.inv);
  }
  double e = 0.0, mx = -INFINITY;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float nv = nm.mode == PI_ONEHOT ? (i == hot ? 1.f : 0.f) : nm.mode == PI_SIGN ? pi_sign(s[i]) : s[i] / nrm;
    const double d = (double)nv - (double)vec[i];
    e += d * d;
    mx = fmax(mx, (double)nv);
    vec[i] = nv;
  }
  e = block_reduce_sum(e, red);
  mx = block_reduce_max(mx, red);
  if (threadIdx.x == 0) {
    part_e[blockIdx.x] = e;
    part_m[blockIdx.x] = mx;
  }
}

// scratch: PI_SCR doubles = [0, NB) |x|^2 partials or maxima, [NB, 2NB) err partials, [2NB, 3NB) max partials,
// [3NB, 4NB) argmax indices, [4NB, 5NB) power sums
constexpr int PI_SCR = 5 * PI_NB;
static void pi_launch_normalize(float* sv, float* vec, long n, PIState* st, int which, const PINorm& nm, double* scr,
                                hipStream_t s) {
  if (nm.mode != PI_L2) {
    if (n < PI_MULTI_MIN) {
      hipLaunchKernelGGL(pi_normalize_p, dim3(1), dim3(1024), 0, s, sv, vec, n, st, which, nm);
      return;
    }
    double *pa = scr, *pe = scr + PI_NB, *pm = scr + 2 * PI_NB, *pidx = scr + 3 * PI_NB, *ps = scr + 4 * PI_NB;
    if (nm.mode != PI_SIGN) hipLaunchKernelGGL(pi_amax_part, dim3(PI_NB), dim3(256), 0, s, sv, n, st, pa, pidx);
    if (nm.mode == PI_POWER) hipLaunchKernelGGL(pi_pow_part, dim3(PI_NB), dim3(256), 0, s, sv, n, st, nm, pa, pidx, ps);
    hipLaunchKernelGGL(pi_apply_p, dim3(PI_NB), dim3(256), 0, s, sv, vec, n, st, nm, pa, pidx, ps, pe, pm);
    hipLaunchKernelGGL(pi_norm_final, dim3(1), dim3(256), 0, s, n, PI_NB, st, pe, pm, which);
    return;
  }
  if (n < PI_MULTI_MIN) {
    hipLaunchKernelGGL(pi_normalize, dim3(1), dim3(1024), 0, s, sv, vec, n, st, which);
    return;
  }
  hipLaunchKernelGGL(pi_dot_part, dim3(PI_NB), dim3(256), 0, s, sv, sv, n, st, scr);
  hipLaunchKernelGGL(pi_norm_apply, dim3(PI_NB), dim3(256), 0, s, sv, vec, n, st, scr, scr + PI_NB, scr + 2 * PI_NB);
  hipLaunchKernelGGL(pi_norm_final, dim3(1), dim3(256), 0, s, n, PI_NB, st, scr + PI_NB, scr + 2 * PI_NB, which);
}

__global__ void pi_init(PIState* st, int use_tol, float atol, float rtol) {
  st->done = 0;
  st->iters = 0;
  st->use_tol = use_tol;
  st->atol = atol;
  st->rtol = rtol;
  st->err_u = 0.0;
  st->max_u = 0.0;
  st->sigma = 0.0;
}

// sigma = u . (W v) (fixed order per thread, fp64)
__global__ __launch_bounds__(1024) void pi_sigma(const float* u, const float* wv, long n, PIState* st, float* scale) {
  __shared__ double red[16];
  double s = 0.0;
  for (long i = threadIdx.x; i < n; i += blockDim.x) s += (double)u[i] * (double)wv[i];
  s = block_reduce_sum(s, red);
  if (threadIdx.x == 0) {
    st->sigma = s;
    if (scale) *scale = (float)s;
  }
}

static PIOp pi_op(const InfPowerIterDesc* d) {
  PIOp op;
  op.W = d->weight;
  op.cin = d->cin;
  op.cout = d->cout;
  const bool spatial = d->kind == INF_LAYER_CONV && d->ksize > 1;
  op.ks = spatial ? d->ksize : 1;
  op.H = spatial ? d->height : 1;
  op.Wd = spatial ? d->width : 1;
  return op;
}

static long pi_nu(const PIOp& op) { return (long)op.cout * op.H * op.Wd; }
static long pi_nv(const PIOp& op) { return (long)op.cin * op.H * op.Wd; }

static int pi_valid(const InfPowerIterDesc* d) {
  if (!d || !d->weight || !d->u || !d->v || d->cin <= 0 || d->cout <= 0) return 0;
  if (d->kind == INF_LAYER_CONV) {
    if (d->ksize < 1 || !(d->ksize & 1)) return 0;
    if (d->ksize > 1 && (d->height <= 0 || d->width <= 0)) return 0;
  } else if (d->kind != INF_LAYER_LINEAR) {
    return 0;
  }
  // induced norms: 0 stands for 2 (a zero-initialised descriptor of an older caller), INFINITY for inf
  for (const float p : {d->domain, d->codomain})
    if (!(p == 0.f || p >= 1.f)) return 0;   // NaN fails both
  return 1;
}

// The reference's 1x1 conv leaves a stored buffer untouched where its normalisation acts on a temporary
// (mixed_lipschitz.py:311-315): v for domain 1, u for codomain inf.  Such a vector is iterated on a copy in the
// workspace and not copied back; sigma still comes from the iterated vectors.
static bool pi_stale_u(const InfPowerIterDesc* d) {
  return d->kind == INF_LAYER_CONV && d->ksize == 1 && std::isinf(d->codomain);
}
static bool pi_stale_v(const InfPowerIterDesc* d) {
  return d->kind == INF_LAYER_CONV && d->ksize == 1 && d->domain == 1.f;
}
static size_t pi_align(size_t b) { return (b + 255) / 256 * 256; }
// after the state(s): W v and W^T u, the reduction scratch, then the copies of the buffers that stay stale
static size_t pi_layer_bytes(const InfPowerIterDesc* d) {
  const PIOp op = pi_op(d);
  const size_t nu = (size_t)pi_nu(op), nv = (size_t)pi_nv(op);
  return pi_align((nu + nv) * sizeof(float)) + pi_align(PI_SCR * sizeof(double)) +
         (pi_stale_u(d) ? pi_align(nu * sizeof(float)) : 0) + (pi_stale_v(d) ? pi_align(nv * sizeof(float)) : 0);
}

struct PILayer {
  PIOp op;
  long nu, nv;
  PINorm nmu, nmv;
  float *us, *vs;   // W v, W^T u
  float *u, *v;     // the iterated vectors: the module's buffers, or workspace copies of them
  double* scr;
};
// carve one layer's workspace (pi_layer_bytes) and queue the copies of the buffers that stay stale
static int pi_layer_setup(const InfPowerIterDesc* d, char* cur, PILayer* l, hipStream_t s) {
  l->op = pi_op(d);
  l->nu = pi_nu(l->op);
  l->nv = pi_nv(l->op);
  l->nmu = pi_norm_of(d->codomain, true);
  l->nmv = pi_norm_of(d->domain, false);
  l->us = reinterpret_cast<float*>(cur);
  l->vs = l->us + l->nu;
  cur += pi_align((size_t)(l->nu + l->nv) * sizeof(float));
  l->scr = reinterpret_cast<double*>(cur);
  cur += pi_align(PI_SCR * sizeof(double));
  l->u = d->u;
  l->v = d->v;
  if (pi_stale_u(d)) {
    l->u = reinterpret_cast<float*>(cur);
    cur += pi_align((size_t)l->nu * sizeof(float));
    INF_HIP(hipMemcpyAsync(l->u, d->u, (size_t)l->nu * sizeof(float), hipMemcpyDeviceToDevice, s));
  }
  if (pi_stale_v(d)) {
    l->v = reinterpret_cast<float*>(cur);
    INF_HIP(hipMemcpyAsync(l->v, d->v, (size_t)l->nv * sizeof(float), hipMemcpyDeviceToDevice, s));
  }
  return INF_OK;
}
static void pi_launch_iteration(const PILayer& l, PIState* st, hipStream_t s) {
  pi_launch_w(l.op, l.v, l.us, st, s);
  pi_launch_normalize(l.us, l.u, l.nu, st, 0, l.nmu, l.scr, s);
  pi_launch_wt(l.op, l.u, l.vs, st, s);
  pi_launch_normalize(l.vs, l.v, l.nv, st, 1, l.nmv, l.scr, s);
}
// sigma = u . (W v)   (mixed_lipschitz.py:126,317,378-380)
static void pi_launch_sigma(const PILayer& l, PIState* st, float* scale, hipStream_t s) {
  pi_launch_w(l.op, l.v, l.us, nullptr, s);
  if (l.nu < PI_MULTI_MIN) {
    hipLaunchKernelGGL(pi_sigma, dim3(1), dim3(1024), 0, s, l.u, l.us, l.nu, st, scale);
  } else {
    hipLaunchKernelGGL(pi_dot_part, dim3(PI_NB), dim3(256), 0, s, l.u, l.us, l.nu, nullptr, l.scr);
    hipLaunchKernelGGL(pi_sigma_final, dim3(1), dim3(256), 0, s, l.scr, PI_NB, st, scale);
  }
}

}  // namespace inf

using namespace inf;

extern "C" {

size_t inf_power_iteration_workspace_bytes(const InfPowerIterDesc* d) {
  if (!pi_valid(d)) return 0;
  return 256 + pi_layer_bytes(d);
}

int inf_power_iteration(const InfPowerIterDesc* d, int max_iters, int use_tol, float atol, float rtol,
                        int* iters_used, void* ws, size_t ws_bytes, void* stream) {
  if (!pi_valid(d) || max_iters < 0) return INF_ERR_INVALID;
  if (!ws || ws_bytes < inf_power_iteration_workspace_bytes(d)) return INF_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  char* base = reinterpret_cast<char*>(ws);
  PIState* st = reinterpret_cast<PIState*>(base);
  PILayer l;
  INF_TRY(pi_layer_setup(d, base + 256, &l, s));
  PIState h;
  memset(&h, 0, sizeof(h));
  hipLaunchKernelGGL(pi_init, dim3(1), dim3(1), 0, s, st, use_tol ? 1 : 0, atol, rtol);
  // speculative chunks of 2, 4, 8, 8, ... iterations between flag reads (a nearly converged u, v, as
  // after one optimiser step, stops within the first chunk)
  int done_iters = 0, chunk = use_tol ? 2 : max_iters;
  while (done_iters < max_iters) {
    const int n = std::min(chunk, max_iters - done_iters);
    for (int k = 0; k < n; ++k) pi_launch_iteration(l, st, s);
    INF_CHECK_LAUNCH();
    done_iters += n;
    chunk = std::min(2 * chunk, 8);
    if (!use_tol) continue;
    INF_HIP(hipMemcpyAsync(&h, st, sizeof(h), hipMemcpyDeviceToHost, s));
    INF_HIP(hipStreamSynchronize(s));
    if (h.done) break;
  }
  pi_launch_sigma(l, st, d->scale, s);
  INF_CHECK_LAUNCH();
  // the count needs no further readback: with the tolerance test the last flag read came after every
  // iteration kernel; without it every iteration runs
  if (iters_used) *iters_used = use_tol ? h.iters : max_iters;
  return INF_OK;
}

// ---- many layers at once (update_lipschitz, train_img.py:786-792): the same per-layer iterations and
// stopping rule, but every unfinished layer's chunk is queued before ONE read-back of all the layers' flags,
// so the host waits once per chunk (<= 5 times for 30 iterations) instead of once per chunk per layer.
size_t inf_power_iteration_batch_workspace_bytes(const InfPowerIterDesc* descs, int n) {
  if (!descs || n <= 0) return 0;
  size_t b = ((sizeof(PIState) * (size_t)n + 255) / 256) * 256;
  for (int i = 0; i < n; ++i) {
    if (!pi_valid(&descs[i])) return 0;
    b += pi_layer_bytes(&descs[i]);
  }
  return b;
}

int inf_power_iteration_batch(const InfPowerIterDesc* descs, int n, int max_iters, int use_tol, float atol,
                              float rtol, int* iters_used, void* ws, size_t ws_bytes, void* stream) {
  if (!descs || n <= 0 || max_iters < 0) return INF_ERR_INVALID;
  for (int i = 0; i < n; ++i)
    if (!pi_valid(&descs[i])) return INF_ERR_INVALID;
  if (!ws || ws_bytes < inf_power_iteration_batch_workspace_bytes(descs, n)) return INF_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  char* base = reinterpret_cast<char*>(ws);
  PIState* states = reinterpret_cast<PIState*>(base);
  char* cur = base + ((sizeof(PIState) * (size_t)n + 255) / 256) * 256;
  std::vector<PILayer> L(n);
  for (int i = 0; i < n; ++i) {
    INF_TRY(pi_layer_setup(&descs[i], cur, &L[i], s));
    cur += pi_layer_bytes(&descs[i]);
    hipLaunchKernelGGL(pi_init, dim3(1), dim3(1), 0, s, states + i, use_tol ? 1 : 0, atol, rtol);
  }
  std::vector<PIState> h(n);
  memset(h.data(), 0, sizeof(PIState) * n);
  std::vector<char> live(n, 1);
  int done_iters = 0, chunk = use_tol ? 2 : max_iters;
  while (done_iters < max_iters) {
    const int c = std::min(chunk, max_iters - done_iters);
    for (int i = 0; i < n; ++i) {
      if (!live[i]) continue;
      for (int k = 0; k < c; ++k) pi_launch_iteration(L[i], states + i, s);
    }
    INF_CHECK_LAUNCH();
    done_iters += c;
    chunk = std::min(2 * chunk, 8);
    if (!use_tol) continue;
    INF_HIP(hipMemcpyAsync(h.data(), states, sizeof(PIState) * n, hipMemcpyDeviceToHost, s));
    INF_HIP(hipStreamSynchronize(s));
    bool any = false;
    for (int i = 0; i < n; ++i) {
      if (h[i].done) live[i] = 0;
      any = any || live[i];
    }
    if (!any) break;
  }
  for (int i = 0; i < n; ++i) pi_launch_sigma(L[i], states + i, descs[i].scale, s);
  INF_CHECK_LAUNCH();
  if (iters_used)
    for (int i = 0; i < n; ++i) iters_used[i] = use_tol ? h[i].iters : max_iters;
  return INF_OK;
}

}  // extern "C"
