// The Broyden solver's device side: the solver's step kernels (the plain step, the line search's trial point, the
// negation), the limited-memory update at every size (one thread per sample, one workgroup per sample, chunked), and the
// per-sample rule's state machine with its Banach fallback.  Maps broyden.py:79,94-99 (line_search's x_est and delta_x),
// :101-120 (rmatvec / matvec), :153-172 (the stopping rules), :174-181 (the update) and implicit_block.py:17-28
// (find_fixed_point).  The step, the stopped sample and the NaN scrub are pointwise_ops.h's; accumulation orders are
// each kernel's own.
#include "pointwise_ops.h"

namespace inf {

// x_est = x0 + update; delta_x = x_est - x0   (line_search(on=False): broyden.py:94-99)
__global__ void axpy_step_kernel(const float* x, const float* upd, float* xnew, float* dx, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  broyden_step(x[i], upd[i], xnew[i], dx[i]);
}
int launch_axpy_step(const float* x, const float* upd, float* xnew, float* dx, long n, hipStream_t s) {
  INF_PROF_LAUNCH(s, 703, 16.0 * n, axpy_step_kernel, dim3((n + 255) / 256), dim3(256), 0, s, x, upd, xnew, dx, n);
  return INF_OK;
}
// line_search(on=True)'s trial point x_est = x0 + s * update and delta_x = x_est - x0 (broyden.py:79,94,99): the product
// and the sum rounded separately, as the reference's two tensor ops do.  The file is built with -ffp-contract=fast, under
// which HIP's __fmul_rn / __fadd_rn are a plain product and sum that the back end contracts into one v_fma_f32 (a
// contract(off) pragma does not stop it either); the empty asm makes the rounded product opaque to that contraction.
__global__ void line_step_kernel(const float* x, const float* upd, float sc, float* xnew, float* dx, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float x0 = x[i];
  float prod = sc * upd[i];
  asm volatile("" : "+v"(prod));
  broyden_step(x0, prod, xnew[i], dx[i]);
}
int launch_line_step(const float* x, const float* upd, float sc, float* xnew, float* dx, long n, hipStream_t s) {
  INF_PROF_LAUNCH(s, 707, 16.0 * n, line_step_kernel, dim3((n + 255) / 256), dim3(256), 0, s, x, upd, sc, xnew, dx, n);
  return INF_OK;
}
__global__ void neg_kernel(const float* x, float* y, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = -x[i];
}
int launch_neg(const float* x, float* y, long n, hipStream_t s) {
  INF_PROF_LAUNCH(s, 704, 8.0 * n, neg_kernel, dim3((n + 255) / 256), dim3(256), 0, s, x, y, n);
  return INF_OK;
}

// ------------------------------------------------------------------------------------------
// Broyden low-rank update (broyden.py:174-181) with H = -I + U V^T:
//   a_j = dx.U_j, c_j = VT_j.dg      (j < m)
//   vT  = -dx + sum_j a_j VT_j                  (rmatvec, :101-109)
//   u   = (dx - (-dg + sum_j c_j U_j)) / (vT.dg)   (matvec, :112-120)
//   NaN -> 0 in vT and u; store column m
//   e_j = VT_j.gx (j < ncols);  update = -(-gx + sum_j e_j U_j);  x_new = x + update
// ------------------------------------------------------------------------------------------
constexpr int BR_CH = 1024;   // elements per block (256 threads x 4)
constexpr int BR_TMAX = 64;

// one thread per sample (small d: fc nets)
__global__ __launch_bounds__(256) void broyden_small_kernel(BroydenArgs a) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.batch) return;
  if (a.active && !a.active[b]) {       // per-sample mode: a stopped sample keeps its iterate and its U / VT
    for (int i = 0; i < a.d; ++i) {
      const long e = br_idx(a, b, i);
      keep_iterate(a, e);
    }
    return;
  }
  float aj[BR_TMAX], cj[BR_TMAX];
  for (int j = 0; j < a.m; ++j) {
    const float* U = a.U + (long)j * a.cs;
    const float* V = a.VT + (long)j * a.cs;
    double sa = 0.0, sc = 0.0;
    for (int i = 0; i < a.d; ++i) {
      const long e = br_idx(a, b, i);
      sa += (double)a.dx[e] * U[e];
      sc += (double)V[e] * a.dg[e];
    }
    aj[j] = (float)sa;
    cj[j] = (float)sc;
  }
  float* Um = a.U + (long)a.m * a.cs;
  float* Vm = a.VT + (long)a.m * a.cs;
  double den = 0.0;
  for (int i = 0; i < a.d; ++i) {
    const long e = br_idx(a, b, i);
    float vt = -a.dx[e], t = -a.dg[e];
    for (int j = 0; j < a.m; ++j) {
      vt += aj[j] * a.VT[(long)j * a.cs + e];
      t += cj[j] * a.U[(long)j * a.cs + e];
    }
    Vm[e] = vt;
    Um[e] = a.dx[e] - t;
    den += (double)vt * a.dg[e];
  }
  const float denf = (float)den;
  for (int i = 0; i < a.d; ++i) {
    const long e = br_idx(a, b, i);
    float vt = Vm[e];
    float u = Um[e] / denf;
    scrub_nan(vt, u);
    Vm[e] = vt;
    Um[e] = u;
  }
  float ej[BR_TMAX];
  for (int j = 0; j < a.ncols; ++j) {
    const float* V = a.VT + (long)j * a.cs;
    double se = 0.0;
    for (int i = 0; i < a.d; ++i) se += (double)V[br_idx(a, b, i)] * a.gx[br_idx(a, b, i)];
    ej[j] = (float)se;
  }
  for (int i = 0; i < a.d; ++i) {
    const long e = br_idx(a, b, i);
    float t = -a.gx[e];
    for (int j = 0; j < a.ncols; ++j) t += ej[j] * a.U[(long)j * a.cs + e];
    store_update(a, e, -t);
  }
}

// the same update for a compile-time d (the tabular / toy nets): one pass over the old columns computes a_j, c_j and
// folds them into vt and t as soon as they are known (the generic kernel's second pass re-reads the columns), and one
// pass over the used columns does the same for e_j, with the new column m from registers.  Every sum runs in the same
// order and precision as broyden_small_kernel (bit-identical); the columns' loads are independent across j, so they
// overlap instead of forming one dependent round trip per column.
template <int DD>
__global__ __launch_bounds__(256) void broyden_small_d_kernel(BroydenArgs a) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.batch) return;
  if (a.active && !a.active[b]) {
#pragma unroll
    for (int i = 0; i < DD; ++i) {
      const long e = br_idx(a, b, i);
      keep_iterate(a, e);
    }
    return;
  }
  float dx[DD], dg[DD], vt[DD], t[DD];
#pragma unroll
  for (int i = 0; i < DD; ++i) {
    const long e = br_idx(a, b, i);
    dx[i] = a.dx[e];
    dg[i] = a.dg[e];
    vt[i] = -dx[i];
    t[i] = -dg[i];
  }
#pragma unroll 4
  for (int j = 0; j < a.m; ++j) {
    const float* U = a.U + (long)j * a.cs;
    const float* V = a.VT + (long)j * a.cs;
    float u[DD], v[DD];
    double sa = 0.0, sc = 0.0;
#pragma unroll
    for (int i = 0; i < DD; ++i) {
      const long e = br_idx(a, b, i);
      u[i] = U[e];
      v[i] = V[e];
    }
#pragma unroll
    for (int i = 0; i < DD; ++i) {
      sa += (double)dx[i] * u[i];
      sc += (double)v[i] * dg[i];
    }
    const float aj = (float)sa, cj = (float)sc;
#pragma unroll
    for (int i = 0; i < DD; ++i) {
      vt[i] += aj * v[i];
      t[i] += cj * u[i];
    }
  }
  float* Um = a.U + (long)a.m * a.cs;
  float* Vm = a.VT + (long)a.m * a.cs;
  float um[DD];
  double den = 0.0;
#pragma unroll
  for (int i = 0; i < DD; ++i) {
    um[i] = dx[i] - t[i];
    den += (double)vt[i] * dg[i];
  }
  const float denf = (float)den;
#pragma unroll
  for (int i = 0; i < DD; ++i) {
    const long e = br_idx(a, b, i);
    float u = um[i] / denf;
    scrub_nan(vt[i], u);
    um[i] = u;
    Vm[e] = vt[i];
    Um[e] = u;
  }
  float gx[DD], tt[DD];
#pragma unroll
  for (int i = 0; i < DD; ++i) {
    gx[i] = a.gx[br_idx(a, b, i)];
    tt[i] = -gx[i];
  }
#pragma unroll 4
  for (int j = 0; j < a.ncols; ++j) {
    float u[DD], v[DD];
    if (j == a.m) {
#pragma unroll
      for (int i = 0; i < DD; ++i) {
        u[i] = um[i];
        v[i] = vt[i];
      }
    } else {
      const float* U = a.U + (long)j * a.cs;
      const float* V = a.VT + (long)j * a.cs;
#pragma unroll
      for (int i = 0; i < DD; ++i) {
        const long e = br_idx(a, b, i);
        u[i] = U[e];
        v[i] = V[e];
      }
    }
    double se = 0.0;
#pragma unroll
    for (int i = 0; i < DD; ++i) se += (double)v[i] * gx[i];
    const float ej = (float)se;
#pragma unroll
    for (int i = 0; i < DD; ++i) tt[i] += ej * u[i];
  }
#pragma unroll
  for (int i = 0; i < DD; ++i) {
    const long e = br_idx(a, b, i);
    store_update(a, e, -tt[i]);
  }
}

// chunked multi-kernel version (large d: conv nets), grid (nchunk, B), 256 threads
// part layout: [B][nchunk][2*T] for phase 1, [B][nchunk] (+ offset) for phase 2, [B][nchunk][T] for phase 3
__global__ __launch_bounds__(256) void broyden_p1(BroydenArgs a, int nchunk) {
  __shared__ double red[16];
  const int b = blockIdx.y, ch = blockIdx.x;
  if (a.active && !a.active[b]) return;
  const int lo = ch * BR_CH, hi = min(a.d, lo + BR_CH);
  double* out = a.part + ((long)b * nchunk + ch) * 2 * a.T;
  for (int j = 0; j < a.m; ++j) {
    const float* U = a.U + (long)j * a.cs;
    const float* V = a.VT + (long)j * a.cs;
    double sa = 0.0, sc = 0.0;
    for (int i = lo + threadIdx.x; i < hi; i += blockDim.x) {
      const long e = br_idx(a, b, i);
      sa += (double)a.dx[e] * U[e];
      sc += (double)V[e] * a.dg[e];
    }
    sa = block_sum(sa, red);
    sc = block_sum(sc, red);
    if (threadIdx.x == 0) {
      out[j] = sa;
      out[a.T + j] = sc;
    }
  }
}

// Large d (CelebA-HQ: 192 chunks per sample): the chunk partials are summed once per sample into chunk 0's slot instead
// of by every block of the sample (each of 192 blocks re-summed all 192 partials); the consumers then read nsum = 1.
// One wave per (sample, column): lanes over the chunks, a fixed shuffle tree (deterministic; a serial loop per column
// took 42 us per call).  part[b][c][ld]: column col(j) = j < m1 ? j : off2 + j - m1, j < ncol
__global__ __launch_bounds__(64) void br_sum_chunks(double* part, int nchunk, int ld, int m1, int off2, int ncol,
                                                    const int* active) {
  const int b = blockIdx.x, j = blockIdx.y, lane = threadIdx.x;
  if (j >= ncol || (active && !active[b])) return;
  const int col = j < m1 ? j : off2 + (j - m1);
  double* p = part + (long)b * nchunk * ld + col;
  double s = 0.0;
  for (int c = lane; c < nchunk; c += 64) s += p[(long)c * ld];
  s = wave_sum(s);
  if (lane == 0) p[0] = s;
}

__global__ __launch_bounds__(256) void broyden_p2(BroydenArgs a, int nchunk, int nsum, double* part2) {
  __shared__ double red[16];
  __shared__ float coef[2 * BR_TMAX];
  const int b = blockIdx.y, ch = blockIdx.x;
  if (a.active && !a.active[b]) return;
  for (int j = threadIdx.x; j < 2 * a.m; j += blockDim.x) {
    const int jj = j < a.m ? j : a.T + (j - a.m);
    double s = 0.0;
    for (int c = 0; c < nsum; ++c) s += a.part[((long)b * nchunk + c) * 2 * a.T + jj];
    coef[j] = (float)s;   // a_j (j < m) then c_j
  }
  __syncthreads();
  const int lo = ch * BR_CH, hi = min(a.d, lo + BR_CH);
  float* Um = a.U + (long)a.m * a.cs;
  float* Vm = a.VT + (long)a.m * a.cs;
  double den = 0.0;
  for (int i = lo + threadIdx.x; i < hi; i += blockDim.x) {
    const long e = br_idx(a, b, i);
    float vt = -a.dx[e], t = -a.dg[e];
    for (int j = 0; j < a.m; ++j) {
      vt += coef[j] * a.VT[(long)j * a.cs + e];
      t += coef[a.m + j] * a.U[(long)j * a.cs + e];
    }
    Vm[e] = vt;
    Um[e] = a.dx[e] - t;
    den += (double)vt * a.dg[e];
  }
  den = block_sum(den, red);
  if (threadIdx.x == 0) part2[(long)b * nchunk + ch] = den;
}

__global__ __launch_bounds__(256) void broyden_p3(BroydenArgs a, int nchunk, int nsum, const double* part2, double* part3) {
  __shared__ double red[16];
  __shared__ float denf;
  const int b = blockIdx.y, ch = blockIdx.x;
  if (a.active && !a.active[b]) return;
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int c = 0; c < nsum; ++c) s += part2[(long)b * nchunk + c];
    denf = (float)s;
  }
  __syncthreads();
  const int lo = ch * BR_CH, hi = min(a.d, lo + BR_CH);
  float* Um = a.U + (long)a.m * a.cs;
  float* Vm = a.VT + (long)a.m * a.cs;
  for (int i = lo + threadIdx.x; i < hi; i += blockDim.x) {
    const long e = br_idx(a, b, i);
    float vt = Vm[e];
    float u = Um[e] / denf;
    scrub_nan(vt, u);
    Vm[e] = vt;
    Um[e] = u;
  }
  __syncthreads();
  double* out = part3 + ((long)b * nchunk + ch) * a.T;
  for (int j = 0; j < a.ncols; ++j) {
    const float* V = a.VT + (long)j * a.cs;
    double se = 0.0;
    for (int i = lo + threadIdx.x; i < hi; i += blockDim.x) {
      const long e = br_idx(a, b, i);
      se += (double)V[e] * a.gx[e];
    }
    se = block_sum(se, red);
    if (threadIdx.x == 0) out[j] = se;
  }
}

__global__ __launch_bounds__(256) void broyden_p4(BroydenArgs a, int nchunk, int nsum, const double* part3) {
  __shared__ float ej[BR_TMAX];
  const int b = blockIdx.y, ch = blockIdx.x;
  if (a.active && !a.active[b]) {
    const int lo = ch * BR_CH, hi = min(a.d, lo + BR_CH);
    for (int i = lo + threadIdx.x; i < hi; i += blockDim.x) {
      const long e = br_idx(a, b, i);
      keep_iterate(a, e);
    }
    return;
  }
  for (int j = threadIdx.x; j < a.ncols; j += blockDim.x) {
    double s = 0.0;
    for (int c = 0; c < nsum; ++c) s += part3[((long)b * nchunk + c) * a.T + j];
    ej[j] = (float)s;
  }
  __syncthreads();
  const int lo = ch * BR_CH, hi = min(a.d, lo + BR_CH);
  for (int i = lo + threadIdx.x; i < hi; i += blockDim.x) {
    const long e = br_idx(a, b, i);
    float t = -a.gx[e];
    for (int j = 0; j < a.ncols; ++j) t += ej[j] * a.U[(long)j * a.cs + e];
    store_update(a, e, -t);
  }
}

// The whole update in one launch for d <= BR_FUSED_CH chunks (CIFAR-10: d = 3072, 3 chunks): one workgroup per sample;
// its thread group g (256 threads) does for chunk g exactly what one block of broyden_p1..p4 does (same elements per
// thread, same accumulation order, the same wave sums added in wave order for the chunk's block sum, the chunk sums in
// chunk order), so the results are bitwise those of the four launches.  The chunk partials stay in LDS, and U_m / VT_m
// and this thread's d-vector elements stay in registers between the stages (the three launches in between, each
// waiting for CUs beside the other branch's series in the overlapped schedule, are gone).
constexpr int BR_FUSED_CH = 4;
__global__ __launch_bounds__(256 * BR_FUSED_CH) void broyden_fused_kernel(BroydenArgs a, int nchunk) {
  constexpr int PER = BR_CH / 256;                   // elements per thread and chunk (as in the chunked kernels)
  __shared__ double ws[4 * BR_FUSED_CH][2 * BR_TMAX];
  __shared__ float coef[2 * BR_TMAX];
  __shared__ float denf;
  const int b = blockIdx.x;
  const int g = threadIdx.x >> 8, tg = threadIdx.x & 255, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int lo = g * BR_CH, hi = min(a.d, lo + BR_CH);
  long e[PER];
  bool ok[PER];
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int i = lo + tg + 256 * k;
    ok[k] = i < hi;
    e[k] = br_idx(a, b, ok[k] ? i : lo);
  }
  if (a.active && !a.active[b]) {                    // (broyden_p4's stopped sample; p1..p3 skip it)
#pragma unroll
    for (int k = 0; k < PER; ++k)
      if (ok[k]) {
        keep_iterate(a, e[k]);
      }
    return;
  }
  float dx[PER], dg[PER], gx[PER];
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    dx[k] = ok[k] ? a.dx[e[k]] : 0.f;
    dg[k] = ok[k] ? a.dg[e[k]] : 0.f;
    gx[k] = ok[k] ? a.gx[e[k]] : 0.f;
  }
  // chunk sum of column jj from the per-wave sums: the chunk's 4 waves in order, then the chunks in order
  auto csum = [&](int jj) {
    double s = 0.0;
    for (int c = 0; c < nchunk; ++c) {
      double r = 0.0;
#pragma unroll
      for (int i = 0; i < 4; ++i) r += ws[4 * c + i][jj];
      s += r;
    }
    return s;
  };
  // p1: a_j = dx . U_j, c_j = VT_j . dg (j < m)
  for (int j = 0; j < a.m; ++j) {
    const float* U = a.U + (long)j * a.cs;
    const float* V = a.VT + (long)j * a.cs;
    double sa = 0.0, sc = 0.0;
#pragma unroll
    for (int k = 0; k < PER; ++k)
      if (ok[k]) {
        sa += (double)dx[k] * U[e[k]];
        sc += (double)V[e[k]] * dg[k];
      }
    sa = wave_sum(sa);
    sc = wave_sum(sc);
    if (lane == 0) {
      ws[w][j] = sa;
      ws[w][BR_TMAX + j] = sc;
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < 2 * a.m; j += blockDim.x) coef[j] = (float)csum(j < a.m ? j : BR_TMAX + (j - a.m));
  __syncthreads();
  // p2: VT_m, U_m and the denominator
  float vt[PER], um[PER];
  double den = 0.0;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    if (!ok[k]) continue;
    float v_ = -dx[k], t = -dg[k];
    for (int j = 0; j < a.m; ++j) {
      v_ += coef[j] * a.VT[(long)j * a.cs + e[k]];
      t += coef[a.m + j] * a.U[(long)j * a.cs + e[k]];
    }
    vt[k] = v_;
    um[k] = dx[k] - t;
    den += (double)v_ * dg[k];
  }
  den = wave_sum(den);
  if (lane == 0) ws[w][0] = den;
  __syncthreads();
  if (threadIdx.x == 0) denf = (float)csum(0);
  __syncthreads();
  // p3: scale U_m, scrub NaN, store U_m / VT_m; e_j = VT_j . gx (j < ncols; VT_m from registers)
  float* Um = a.U + (long)a.m * a.cs;
  float* Vm = a.VT + (long)a.m * a.cs;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    if (!ok[k]) continue;
    float v_ = vt[k];
    float u = um[k] / denf;
    scrub_nan(v_, u);
    vt[k] = v_;
    um[k] = u;
    Vm[e[k]] = v_;
    Um[e[k]] = u;
  }
  for (int j = 0; j < a.ncols; ++j) {
    const float* V = a.VT + (long)j * a.cs;
    double se = 0.0;
#pragma unroll
    for (int k = 0; k < PER; ++k)
      if (ok[k]) se += (double)(j == a.m ? vt[k] : V[e[k]]) * gx[k];
    se = wave_sum(se);
    if (lane == 0) ws[w][j] = se;
  }
  __syncthreads();
  for (int j = threadIdx.x; j < a.ncols; j += blockDim.x) coef[j] = (float)csum(j);
  __syncthreads();
  // p4: update = -(-gx + sum_j e_j U_j), x_new, dx_new
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    if (!ok[k]) continue;
    float t = -gx[k];
    for (int j = 0; j < a.ncols; ++j) t += coef[j] * (j == a.m ? um[k] : a.U[(long)j * a.cs + e[k]]);
    store_update(a, e[k], -t);
  }
}

int launch_broyden_update(const BroydenArgs& a, hipStream_t s) {
  if (a.T > BR_TMAX || a.m >= a.T || a.ncols > a.T) return INF_ERR_INVALID;
  // algorithmic bytes (fp32, D = batch x d): each kernel's distinct reads and writes of the d-vectors and U / VT columns
  const double D4 = 4.0 * a.batch * a.d;
  if (a.d <= 32) {
    // dx, dg, gx, x; U_j, VT_j for j < ncols, j != m; writes U_m, VT_m, update, x_new, dx_new
    const double by = D4 * (9.0 + 2.0 * (a.ncols > 0 ? a.ncols - 1 : 0));
    const dim3 g((a.batch + 255) / 256);
    if (a.d == 2) INF_PROF_LAUNCH(s, 715, by, broyden_small_d_kernel<2>, g, dim3(256), 0, s, a);
    else if (a.d == 6) INF_PROF_LAUNCH(s, 715, by, broyden_small_d_kernel<6>, g, dim3(256), 0, s, a);
    else if (a.d == 8) INF_PROF_LAUNCH(s, 715, by, broyden_small_d_kernel<8>, g, dim3(256), 0, s, a);
    else INF_PROF_LAUNCH(s, 715, by, broyden_small_kernel, g, dim3(256), 0, s, a);
    return INF_OK;
  }
  const int nchunk = (a.d + BR_CH - 1) / BR_CH;
  if (nchunk <= BR_FUSED_CH) {
    // dx, dg, gx, x; U_j, VT_j (j < m); writes U_m, VT_m, update, x_new, dx_new
    INF_PROF_LAUNCH(s, 716, D4 * (9.0 + 2.0 * a.m), broyden_fused_kernel, dim3(a.batch), dim3(256 * nchunk), 0, s, a,
                    nchunk);
    return INF_OK;
  }
  dim3 grid(nchunk, a.batch);
  double* part2 = a.part + (long)a.batch * nchunk * 2 * a.T;
  double* part3 = part2 + (long)a.batch * nchunk;
  const bool pre = nchunk >= 32;       // (small nchunk: the consumers' own sums are cheaper than three more launches)
  const int nsum = pre ? 1 : nchunk;
  const double P8 = 8.0 * a.batch * nchunk;   // one fp64 partial per (sample, chunk)
  if (a.m > 0) {
    // a_j = dx.U_j, c_j = VT_j.dg: dx, dg, U_j, VT_j (j < m)
    INF_PROF_LAUNCH(s, 710, D4 * (2.0 + 2.0 * a.m) + P8 * 2 * a.m, broyden_p1, grid, dim3(256), 0, s, a, nchunk);
    if (pre)
      INF_PROF_LAUNCH(s, 714, P8 * 2 * a.m + 8.0 * a.batch * 2 * a.m, br_sum_chunks, dim3(a.batch, 2 * a.m), dim3(64),
                      0, s, a.part, nchunk, 2 * a.T, a.m, a.T, 2 * a.m, a.active);
  }
  // VT_m, U_m and the denominator: dx, dg, U_j, VT_j (j < m); writes U_m, VT_m
  INF_PROF_LAUNCH(s, 711, D4 * (4.0 + 2.0 * a.m) + P8, broyden_p2, grid, dim3(256), 0, s, a, nchunk, nsum, part2);
  if (pre) INF_PROF_LAUNCH(s, 714, P8 + 8.0 * a.batch, br_sum_chunks, dim3(a.batch, 1), dim3(64), 0, s, part2, nchunk, 1, 1, 0, 1, a.active);
  // scale U_m (read / write U_m, VT_m) and e_j = VT_j.gx: VT_j (j < ncols, j != m), gx
  INF_PROF_LAUNCH(s, 712, D4 * (4.0 + a.ncols) + P8 * a.ncols, broyden_p3, grid, dim3(256), 0, s, a, nchunk, nsum,
                  part2, part3);
  if (pre && a.ncols > 0)
    INF_PROF_LAUNCH(s, 714, P8 * a.ncols + 8.0 * a.batch * a.ncols, br_sum_chunks, dim3(a.batch, a.ncols), dim3(64), 0,
                    s, part3, nchunk, a.T, a.ncols, 0, a.ncols, a.active);
  // update = -(-gx + sum_j e_j U_j), x_new, dx_new: gx, x, U_j (j < ncols); writes update, x_new, dx_new
  INF_PROF_LAUNCH(s, 713, D4 * (5.0 + a.ncols), broyden_p4, grid, dim3(256), 0, s, a, nchunk, nsum, part3);
  return INF_OK;
}

// ------------------------------------------------------------------------------------------
// Per-sample convergence (INF_CONV_PER_SAMPLE): every sample runs the reference's stopping rules
// (broyden.py:153-172) on its own residual norm against eps * sqrt(d), i.e. exactly what broyden() returns
// for a batch of one.  All samples advance in lockstep launches; the state machine lives on the device, so a
// speculatively queued iteration (engine.hip broyden_core) already sees the decisions of the one before it.
// state[b * (PS_HEAD + T) + ...]: 0 init, 1 lowest, 2 -, 3 nstep, 4 lowest_step, 5 prot_break, 6 latest,
// PS_HEAD.. the ring of the last T objectives (step k at (k - 1) % T).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void ps_decide_kernel(double* ss, double* state, int* active, int* improved,
                                                         int B, int k, int T, double eps) {
  __shared__ double red[16];
  double cnt = 0.0;
  const int stride = PS_HEAD + T;
  for (int b = threadIdx.x; b < B; b += blockDim.x) {
    double* st = state + (long)b * stride;
    const double obj = sqrt(ss[b]);
    int act = 0, imp = 0;
    if (k == 0) {                                          // broyden.py:145-153
      st[0] = obj;
      st[1] = obj;
      st[3] = 0.0;
      st[4] = 0.0;
      st[5] = 0.0;
      st[6] = obj;
      act = (obj >= eps && T > 0) ? 1 : 0;
      imp = 1;                                             // lowest_xest = x0
    } else if (active[b]) {
      st[3] = k;
      st[6] = obj;
      st[PS_HEAD + (k - 1) % T] = obj;
      if (obj < st[1]) {                                   // :159-162
        st[1] = obj;
        st[4] = k;
        imp = 1;
      }
      act = 1;
      if (obj < eps) {                                     // :163
        act = 0;
      } else {
        if (obj < 3 * eps && k == T) {                     // :165-168 (trace[-T:] = steps 1..T)
          double mx = st[PS_HEAD], mn = st[PS_HEAD];
          for (int j = 1; j < T; ++j) {
            mx = fmax(mx, st[PS_HEAD + j]);
            mn = fmin(mn, st[PS_HEAD + j]);
          }
          if (mx / mn < 1.3) act = 0;
        }
        if (act && obj > st[0] * 1e6) {                    // :169-172
          st[5] = 1.0;
          act = 0;
        }
        if (k >= T) act = 0;                               // :153
      }
    }
    active[b] = act;
    improved[b] = imp;
    cnt += act;
  }
  cnt = block_sum(cnt, red);
  if (threadIdx.x == 0) ss[B] = cnt;
}
int launch_ps_decide(double* ss, double* state, int* active, int* improved, int B, int k, int T, double eps,
                     hipStream_t s) {
  hipLaunchKernelGGL(ps_decide_kernel, dim3(1), dim3(1024), 0, s, ss, state, active, improved, B, k, T, eps);
  INF_CHECK_LAUNCH();
  return INF_OK;
}
// lowest iterate (and its f) of the improved samples: grid (chunks, B)
__global__ __launch_bounds__(256) void ps_copy_kernel(const int* improved, const float* x, const float* f,
                                                      float* lowx, float* lowf, int d, long sb, long si) {
  const int b = blockIdx.y;
  if (!improved[b]) return;
  for (int i = blockIdx.x * 1024 + threadIdx.x; i < min(d, (int)(blockIdx.x + 1) * 1024); i += blockDim.x) {
    const long e = (long)b * sb + (long)i * si;
    lowx[e] = x[e];
    if (f) lowf[e] = f[e];
  }
}
int launch_ps_copy(const int* improved, const float* x, const float* f, float* lowx, float* lowf, int B, int d, long sb,
                   long si, hipStream_t s) {
  hipLaunchKernelGGL(ps_copy_kernel, dim3((d + 1023) / 1024, B), dim3(256), 0, s, improved, x, f, lowx, lowf, d, sb,
                     si);
  INF_CHECK_LAUNCH();
  return INF_OK;
}
// Banach fallback per sample (find_fixed_point, implicit_block.py:17-28, on a batch of one): for every sample
// still iterating (todo[b]), test sum_i [(x - xp)^2 / (eps + eps |y|) >= 1] == 0; a sample that passes (or every
// remaining one when `force`) takes x as its result and stops.  One workgroup per sample.
__global__ __launch_bounds__(256) void ps_fixed_point_kernel(const float* x, const float* xp, const float* y,
                                                             float* result, int* todo, int d, long sb, long si,
                                                             float eps, int force) {
  __shared__ double red[16];
  const int b = blockIdx.x;
  if (!todo[b]) return;
  double bad = 0.0;
  for (int i = threadIdx.x; i < d; i += blockDim.x) {
    const long e = (long)b * sb + (long)i * si;
    const float dd = x[e] - xp[e];
    const float tol = eps + eps * fabsf(y[e]);
    bad += !((dd * dd) / tol < 1.f) ? 1.0 : 0.0;
  }
  bad = block_sum(bad, red);
  if (bad == 0.0 || force) {
    for (int i = threadIdx.x; i < d; i += blockDim.x) {
      const long e = (long)b * sb + (long)i * si;
      result[e] = x[e];
    }
    __syncthreads();
    if (threadIdx.x == 0) todo[b] = 0;
  }
}
int launch_ps_fixed_point(const float* x, const float* xp, const float* y, float* result, int* todo, int B, int d,
                          long sb, long si, float eps, int force, hipStream_t s) {
  hipLaunchKernelGGL(ps_fixed_point_kernel, dim3(B), dim3(256), 0, s, x, xp, y, result, todo, d, sb, si, eps, force);
  INF_CHECK_LAUNCH();
  return INF_OK;
}

}  // namespace inf
