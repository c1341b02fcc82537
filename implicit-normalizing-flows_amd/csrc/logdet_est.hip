// The log-det estimators' device side for fc nets and the series combine: the exact log|det(I + J)| of a small
// Jacobian, the exact-trace power series, the three estimators' gradients as stacked (A, b) pairs (from J for d <= 16,
// from the two chains for any width), the sum over the pairs, the forward-mode activation that builds J, and the
// combine of the Hutchinson series' per-term partials.  Maps implicit_block.py:249-260 (batch_jacobian + torch.logdet),
// :323-343 (exact_trace), :418-426 (basic_logdet_estimator) and iresblock.py:150-157.
#include "kernels.h"

namespace inf {

// power-series coefficients, passed by value as a kernel argument: c[k] = coeff_host[k] for k < n_terms <= 128, else 0
struct CoeffTable {
  float c[128];
};
static CoeffTable make_coeff_table(const float* coeff_host, int n_terms) {
  CoeffTable ct;
  for (int k = 0; k < 128; ++k) ct.c[k] = k < n_terms ? coeff_host[k] : 0.f;
  return ct;
}

// ------------------------------------------------------------------------------------------
// exact log|det(I + T)| per sample (torch.logdet via LU, implicit_block.py:253-258).  T is stored
// feature-major as tangents: T[i][j] of sample b at tang[i * ld + (j + 1) * stride_j + b],
// ld = (d + 1) * stride_j.  det <= 0 follows torch.logdet: NaN for negative, -inf for zero.
// ------------------------------------------------------------------------------------------
__global__ void logdet_small_kernel(const float* tang, float* out, int d, int batch, long stride_j) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  float M[16][16];
  const long ld = (long)(d + 1) * stride_j;
  for (int i = 0; i < d; ++i)
    for (int j = 0; j < d; ++j) M[i][j] = (i == j ? 1.f : 0.f) + tang[i * ld + (j + 1) * stride_j + b];
  float logabs = 0.f;
  int sign = 1;
  for (int k = 0; k < d; ++k) {
    int piv = k;
    float best = fabsf(M[k][k]);
    for (int i = k + 1; i < d; ++i)
      if (fabsf(M[i][k]) > best) { best = fabsf(M[i][k]); piv = i; }
    if (piv != k) {
      for (int j = 0; j < d; ++j) { const float t = M[k][j]; M[k][j] = M[piv][j]; M[piv][j] = t; }
      sign = -sign;
    }
    const float pv = M[k][k];
    if (pv == 0.f) { logabs = -INFINITY; sign = 0; break; }
    if (pv < 0.f) sign = -sign;
    logabs += logf(fabsf(pv));
    for (int i = k + 1; i < d; ++i) {
      const float f = M[i][k] / pv;
      for (int j = k + 1; j < d; ++j) M[i][j] -= f * M[k][j];
    }
  }
  out[b] = sign > 0 ? logabs : (sign == 0 ? -INFINITY : NAN);
}
int launch_logdet_small(const float* tang, float* out, int d, int batch, long stride_j, hipStream_t s) {
  if (d > 16) return INF_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(logdet_small_kernel, dim3((batch + 127) / 128), dim3(128), 0, s, tang, out, d, batch, stride_j);
  INF_CHECK_LAUNCH();
  return INF_OK;
}

// Exact-trace power series (implicit_block.py:323-343, iresblock.py:150-157), one thread per sample:
//   out = tr(J) + sum_{k=2..n} c_k tr(J^k),  J^k = J @ J^(k-1)   (torch.bmm(J, J_k) order)
// with c_k = (-1)^(k+1)/k * coeff_fn(k) (coeff[k-1]; coeff[0] unused: the reference's first term is
// the bare trace).  fp32 throughout, accumulated in k order like the reference.
__global__ void trace_series_kernel(const float* tang, CoeffTable ct, int n_terms, float* out, int d, int batch,
                                    long stride_j) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  float J[16][16], Pk[16][16];
  const long ld = (long)(d + 1) * stride_j;
  float acc = 0.f;
  for (int i = 0; i < d; ++i)
    for (int j = 0; j < d; ++j) {
      J[i][j] = tang[i * ld + (j + 1) * stride_j + b];
      Pk[i][j] = J[i][j];
    }
  for (int i = 0; i < d; ++i) acc += J[i][i];
  for (int k = 2; k <= n_terms; ++k) {
    float T[16][16];
    for (int i = 0; i < d; ++i)
      for (int j = 0; j < d; ++j) {
        float s = 0.f;
        for (int m = 0; m < d; ++m) s = fmaf(J[i][m], Pk[m][j], s);
        T[i][j] = s;
      }
    float tr = 0.f;
    for (int i = 0; i < d; ++i) {
      for (int j = 0; j < d; ++j) Pk[i][j] = T[i][j];
      tr += Pk[i][i];
    }
    acc = acc + ct.c[k - 1] * tr;
  }
  out[b] = acc;
}
int launch_trace_series(const float* tang, const float* coeff_host, int n_terms, float* out, int d, int batch,
                        long stride_j, hipStream_t s) {
  if (d > 16 || n_terms > 128) return INF_ERR_UNSUPPORTED;
  const CoeffTable ct = make_coeff_table(coeff_host, n_terms);
  hipLaunchKernelGGL(trace_series_kernel, dim3((batch + 127) / 128), dim3(128), 0, s, tang, ct, n_terms, out, d,
                     batch, stride_j);
  INF_CHECK_LAUNCH();
  return INF_OK;
}

// ---- the log-det estimators' gradients as pairs (fc nets, engine.hip inf_logdet_grad) -------------------------------
// Every estimator's differential is a sum of bilinear terms in dJ: d S_b = sum_t A_tb^T dJ(x_b) b_tb (dJ over the
// parameters and x), so g_b S_b differentiates as the forward-over-reverse surrogate of the stacked pairs.  Per sample
// (one thread), from its Jacobian J (fc_jacobian's tangent layout) and the upstream gradient g_b:
//   series  S = sum_k c_k eps^T J^k eps (basic_logdet_estimator, implicit_block.py:418-426; c_k = coeff[k-1]):
//           d S = sum_k c_k sum_{j+m=k-1} a_j^T dJ b_m with a_j = (J^T)^j eps, b_m = J^m eps, so the n pairs are
//           A_m = g sum_{j<=n-1-m} c_{j+m+1} a_j, b_m (m < n);
//   logdet  S = log|det(I + J)| (batch_jacobian + torch.logdet, implicit_block.py:249-260): d S = tr((I + J)^-1 dJ), the
//           d pairs A_j = g row j of (I + J)^-1, b_j = e_j;
//   trace   S = sum_k c_k tr(J^k) (exact_trace, :323-343; coeff[0] the bare trace's 1): d S = tr(P dJ),
//           P = sum_k k c_k J^(k-1), the d pairs A_j = g row j of P, b_j = e_j.
// Outputs, column t B + b of (d, T B) feature-major arrays: A, bv, and xr = x (the point each pair is taken at); value[b] = S.
// a_scr: (n, d, B) scratch for the series' left vectors.
__global__ void logdet_pairs_kernel(int mode, const float* tang, const float* eps, const float* x, const float* gout,
                                    CoeffTable ct, int n_terms, int d, int batch, float* A, float* bv, float* xr,
                                    float* value, float* a_scr) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  float J[16][16];
  const long ld = (long)(d + 1) * batch;
  for (int i = 0; i < d; ++i)
    for (int j = 0; j < d; ++j) J[i][j] = tang[i * ld + (j + 1) * (long)batch + b];
  const float g = gout ? gout[b] : 1.f;
  const int T = mode == LOGDET_SERIES ? n_terms : d;
  const long N = (long)T * batch;
  for (int t = 0; t < T; ++t)
    for (int i = 0; i < d; ++i) xr[i * N + (long)t * batch + b] = x[(long)i * batch + b];
  if (mode == LOGDET_SERIES) {
    float e[16], a[16], v[16], wa[16], wv[16];
    for (int i = 0; i < d; ++i) e[i] = a[i] = v[i] = eps[(long)i * batch + b];
    double val = 0.0;
    for (int m = 0; m < n_terms; ++m) {
      for (int i = 0; i < d; ++i) {
        a_scr[((long)m * d + i) * batch + b] = a[i];             // a_m
        bv[i * N + (long)m * batch + b] = v[i];                  // b_m
      }
      for (int i = 0; i < d; ++i) {                             // a_{m+1} = J^T a_m, b_{m+1} = J b_m
        float sa = 0.f, sv = 0.f;
        for (int k = 0; k < d; ++k) {
          sa = fmaf(J[k][i], a[k], sa);
          sv = fmaf(J[i][k], v[k], sv);
        }
        wa[i] = sa;
        wv[i] = sv;
      }
      double dot = 0.0;
      for (int i = 0; i < d; ++i) {
        a[i] = wa[i];
        v[i] = wv[i];
        dot += (double)a[i] * e[i];                             // eps^T J^(m+1) eps
      }
      val += (double)ct.c[m] * dot;
    }
    for (int m = 0; m < n_terms; ++m) {
      float acc[16];
      for (int i = 0; i < d; ++i) acc[i] = 0.f;
      for (int j = 0; j + m < n_terms; ++j) {
        const float c = ct.c[j + m];
        for (int i = 0; i < d; ++i) acc[i] = fmaf(c, a_scr[((long)j * d + i) * batch + b], acc[i]);
      }
      for (int i = 0; i < d; ++i) A[i * N + (long)m * batch + b] = g * acc[i];
    }
    if (value) value[b] = (float)val;
    return;
  }
  float P[16][16];
  double val = 0.0;
  if (mode == LOGDET_EXACT) {
    // (I + J)^-1 by Gauss-Jordan with partial pivoting; log|det| from the pivots
    float M[16][16];
    for (int i = 0; i < d; ++i)
      for (int j = 0; j < d; ++j) {
        M[i][j] = (i == j ? 1.f : 0.f) + J[i][j];
        P[i][j] = i == j ? 1.f : 0.f;
      }
    float logabs = 0.f;
    int sign = 1;
    for (int k = 0; k < d; ++k) {
      int piv = k;
      float best = fabsf(M[k][k]);
      for (int i = k + 1; i < d; ++i)
        if (fabsf(M[i][k]) > best) {
          best = fabsf(M[i][k]);
          piv = i;
        }
      if (piv != k) {
        for (int j = 0; j < d; ++j) {
          float t = M[k][j];
          M[k][j] = M[piv][j];
          M[piv][j] = t;
          t = P[k][j];
          P[k][j] = P[piv][j];
          P[piv][j] = t;
        }
        sign = -sign;
      }
      const float pv = M[k][k];
      if (pv < 0.f) sign = -sign;
      logabs += logf(fabsf(pv));
      const float r = 1.f / pv;
      for (int j = 0; j < d; ++j) {
        M[k][j] *= r;
        P[k][j] *= r;
      }
      for (int i = 0; i < d; ++i) {
        if (i == k) continue;
        const float f = M[i][k];
        for (int j = 0; j < d; ++j) {
          M[i][j] -= f * M[k][j];
          P[i][j] -= f * P[k][j];
        }
      }
    }
    val = sign > 0 ? logabs : NAN;
  } else {
    // P = sum_k k c_k J^(k-1), val = sum_k c_k tr(J^k)
    float Q[16][16];                                             // J^(k-1)
    for (int i = 0; i < d; ++i)
      for (int j = 0; j < d; ++j) {
        Q[i][j] = i == j ? 1.f : 0.f;
        P[i][j] = 0.f;
      }
    for (int k = 1; k <= n_terms; ++k) {
      const float c = ct.c[k - 1];
      float R[16][16];                                           // J^k = J Q
      for (int i = 0; i < d; ++i)
        for (int j = 0; j < d; ++j) {
          P[i][j] = fmaf((float)k * c, Q[i][j], P[i][j]);
          float sm = 0.f;
          for (int q = 0; q < d; ++q) sm = fmaf(J[i][q], Q[q][j], sm);
          R[i][j] = sm;
        }
      double tr = 0.0;
      for (int i = 0; i < d; ++i) {
        for (int j = 0; j < d; ++j) Q[i][j] = R[i][j];
        tr += Q[i][i];
      }
      val += (double)c * tr;
    }
  }
  for (int t = 0; t < d; ++t)
    for (int i = 0; i < d; ++i) {
      A[i * N + (long)t * batch + b] = g * P[t][i];
      bv[i * N + (long)t * batch + b] = i == t ? 1.f : 0.f;
    }
  if (value) value[b] = (float)val;
}
int launch_logdet_pairs(int mode, const float* tang, const float* eps, const float* x, const float* gout,
                        const float* coeff_host, int n_terms, int d, int batch, float* A, float* bv, float* xr,
                        float* value, float* a_scr, hipStream_t s) {
  if (d > 16 || n_terms > 128 || n_terms < 1) return INF_ERR_UNSUPPORTED;
  const CoeffTable ct = make_coeff_table(coeff_host, n_terms);
  hipLaunchKernelGGL(logdet_pairs_kernel, dim3((batch + 63) / 64), dim3(64), 0, s, mode, tang, eps, x, gout, ct, n_terms,
                     d, batch, A, bv, xr, value, a_scr);
  INF_CHECK_LAUNCH();
  return INF_OK;
}
// The series' pairs of an fc net of any width, from the two chains instead of from J (engine_grad.hip series_pairs_chains):
// a (n, d, B) holds a_j = (J^T)^j eps, bs (n + 1, d, B) holds b_m = J^m eps.  The first blocks write element
// e = i N + m B + b of the three (d, N = n B) arrays, one per thread: A = g_b sum_{j<=n-1-m} c_{j+m+1} a_j, bv = b_m,
// xr = x.  The blocks after them (value given) write value[b] = sum_k c_k eps . b_k: 64 samples per block, the d
// features over 4 slices, summed in double in slice order.
constexpr int SPW_SAMPLES = 64, SPW_SLICES = 4;
__global__ __launch_bounds__(256) void series_pairs_wide_kernel(const float* a, const float* bs, const float* x,
                                                                const float* gout, CoeffTable ct, int n_terms, int d,
                                                                int batch, unsigned pair_blocks, float* A, float* bv,
                                                                float* xr, float* value) {
  const size_t N = (size_t)n_terms * batch, dB = (size_t)d * batch;
  if (blockIdx.x < pair_blocks) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)d * N) return;
    const size_t i = e / N, col = e - i * N;
    const int m = (int)(col / batch), b = (int)(col - (size_t)m * batch);
    const size_t ib = i * batch + b;
    float acc = 0.f;
    for (int j = 0; j + m < n_terms; ++j) acc = fmaf(ct.c[j + m], a[(size_t)j * dB + ib], acc);
    A[e] = (gout ? gout[b] : 1.f) * acc;
    bv[e] = bs[(size_t)m * dB + ib];
    xr[e] = x[ib];
    return;
  }
  __shared__ double part[SPW_SLICES][SPW_SAMPLES];
  const int lane = threadIdx.x % SPW_SAMPLES, slice = threadIdx.x / SPW_SAMPLES;
  const long b = (long)(blockIdx.x - pair_blocks) * SPW_SAMPLES + lane;
  double acc = 0.0;
  if (b < batch) {
    const int per = (d + SPW_SLICES - 1) / SPW_SLICES;
    const int i0 = slice * per, i1 = min(d, i0 + per);
    for (int i = i0; i < i1; ++i) {
      const size_t ib = (size_t)i * batch + b;
      const float e = bs[ib];                                    // b_0 = eps
      float t = 0.f;
      for (int k = 1; k <= n_terms; ++k) t = fmaf(ct.c[k - 1], bs[(size_t)k * dB + ib], t);
      acc += (double)e * t;
    }
  }
  part[slice][lane] = acc;
  __syncthreads();
  if (slice == 0 && b < batch) {
    double sum = 0.0;
    for (int q = 0; q < SPW_SLICES; ++q) sum += part[q][lane];
    value[b] = (float)sum;
  }
}
int launch_series_pairs_wide(const float* a, const float* bs, const float* x, const float* gout,
                             const float* coeff_host, int n_terms, int d, int batch, float* A, float* bv, float* xr,
                             float* value, hipStream_t s) {
  if (n_terms > 128 || n_terms < 1 || d < 1 || batch < 1) return INF_ERR_UNSUPPORTED;
  const CoeffTable ct = make_coeff_table(coeff_host, n_terms);
  const size_t ne = (size_t)d * n_terms * batch;
  const size_t pb = (ne + 255) / 256, vb = value ? (size_t)(batch + SPW_SAMPLES - 1) / SPW_SAMPLES : 0;
  if (pb + vb > 0x7fffffffUL) return INF_ERR_INVALID;
  // reads the n a_j per element (n (n + 1) / 2 in all per (i, b)), b_m and x; writes A, bv, xr
  INF_PROF_LAUNCH(s, 722, 4.0 * ne * (0.5 * (n_terms + 1) + 5.0), series_pairs_wide_kernel, dim3((unsigned)(pb + vb)),
                  dim3(256), 0, s, a, bs, x, gout, ct, n_terms, d, batch, (unsigned)pb, A, bv, xr, value);
  return INF_OK;
}
// gx (B, d) boundary layout = sum over the T pairs of the stacked (d, T B) x-gradient
__global__ void sum_pairs_kernel(const float* gs, int T, int d, int batch, float* gx) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long)batch * d) return;
  const int b = (int)(e / d), i = (int)(e - (long)b * d);
  const long N = (long)T * batch;
  float acc = 0.f;
  for (int t = 0; t < T; ++t) acc += gs[i * N + (long)t * batch + b];
  gx[e] = acc;
}
int launch_sum_pairs(const float* gs, int T, int d, int batch, float* gx, hipStream_t s) {
  const long n = (long)batch * d;
  hipLaunchKernelGGL(sum_pairs_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, gs, T, d, batch, gx);
  INF_CHECK_LAUNCH();
  return INF_OK;
}

// forward-mode activation on [primal | ntang tangent blocks], feature-major (d_out, (1+ntang)*B):
// primal a -> act(a), tangents t -> act'(a) * t.
__global__ void fwdmode_act_kernel(float* a, int d_out, int batch, int ntang, int act, const float* beta) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)d_out * batch) return;
  const int m = i / batch, b = i - (long)m * batch;
  const long ld = (long)(ntang + 1) * batch;
  float* row = a + (long)m * ld;
  const float z = row[b];
  float y, dz;
  if (act == ACT_SWISH) {
    const float sp = softplus_f(*beta);
    y = swish_f(z, sp);
    dz = swish_d(z, sp);
  } else if (act == ACT_SIN) {
    y = sinact_f(z);
    dz = sinact_d(z);
  } else {   // the parameter-less kinds (ACT_NONE / ACT_IDENTITY: y = z, dz = 1)
    y = act_any_f(act, z);
    dz = act_any_d(act, z);
  }
  row[b] = y;
  for (int j = 1; j <= ntang; ++j) row[(long)j * batch + b] *= dz;
}
int launch_fwdmode_act(float* a, float* deriv, int d_out, int batch, int ntang, int act, const float* beta,
                       hipStream_t s) {
  (void)deriv;
  const long n = (long)d_out * batch;
  hipLaunchKernelGGL(fwdmode_act_kernel, dim3((n + 255) / 256), dim3(256), 0, s, a, d_out, batch, ntang, act, beta);
  INF_CHECK_LAUNCH();
  return INF_OK;
}

// ------------------------------------------------------------------------------------------
// power-series combine: tr_k[b] = (float) sum_chunks partial[k][b][c];  out[b] = sum_k fl(c_k * tr_k)
// accumulated in fp32 in k order like `logdetgrad = logdetgrad + delta` (implicit_block.py:421-426).
// ------------------------------------------------------------------------------------------
// one 256-thread workgroup per sample: wave w sums terms k = w, w + 4, ... (its lanes over the term's chunks in fp64,
// a fixed shuffle tree) and forms fl(c_k * tr_k); thread 0 then accumulates the terms in k order in fp32, i.e.
// logdetgrad + delta with torch's two roundings per term (CelebA-HQ 256 has 512 chunks per term: a serial loop per
// term took 73 us)
__global__ __launch_bounds__(256) void series_combine_kernel(const double* partials, CoeffTable ct, int n_terms,
                                                             int batch, int nchunk, float* out) {
  const int b = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __shared__ float term[128];
  for (int k = w; k < n_terms; k += 4) {
    const double* p = partials + ((long)k * batch + b) * nchunk;
    double s = 0.0;
    for (int c = lane; c < nchunk; c += 64) s += p[c];
    s = wave_sum(s);
    if (lane == 0) term[k] = ct.c[k] * (float)s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float acc = 0.f;
    for (int j = 0; j < n_terms; ++j) acc = acc + term[j];
    out[b] = acc;
  }
}
int launch_series_combine(const double* partials, const float* coeff_host, int n_terms, int batch, int nchunk,
                          float* out, hipStream_t s) {
  if (n_terms > 128) return INF_ERR_UNSUPPORTED;
  const CoeffTable ct = make_coeff_table(coeff_host, n_terms);
  // the Hutchinson dots' fp64 chunk partials of every term in, one fp32 log-det per sample out
  INF_PROF_LAUNCH(s, 720, 8.0 * batch * nchunk * n_terms + 4.0 * batch, series_combine_kernel, dim3(batch), dim3(256),
                  0, s, partials, ct, n_terms, batch, nchunk, out);
  return INF_OK;
}

}  // namespace inf
