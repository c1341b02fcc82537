// The power-series log-det of a fused fc net pair in one launch (basic_logdet_estimator, implicit_block.py:418-426, for
// the tabular / toy nets in f16x3 arithmetic; the passes are fcblock_pass.h's): fcseries_kernel, fcseries_supported,
// launch_fcseries.  A source fragment: included by fcblock.hip alone, at its end, and compiled in its translation unit
// (see there); it defines non-inline functions, so a second include breaks the one-definition rule.
//
// Workgroup (blockIdx.x, net blockIdx.y) owns 48 samples: one forward pass of f at x keeps act' of every hidden unit in
// registers (SV_SAVE), then term k = 1 .. n: v <- v^T J_f(x) as one pass of the transposed net over the 48 columns
// (SV_VJP: the hidden epilogue multiplies by the saved derivatives), tr_k = v . eps (fp64 sum of the d products), and
// logdet += fl(c_k * (float) tr_k) in fp32 in k order (launch_series_combine's arithmetic).  The operands stay in LDS and
// registers between terms; the only global traffic is x, eps, the out row and the weight planes (L2-resident).
#pragma once

#include "fcblock_pass.h"

namespace inf {

constexpr int FS_LDS = 2 * 2 * BK_S * FC_LD + 4 * 16 * BK_S + 4 * FC_NW * BK_S + 4 * BK_S + 64;
template <int DD, int ACT, int NH>
__global__ __launch_bounds__(FC_NT) void fcseries_kernel(FcSeriesArgs a) {
  __shared__ __attribute__((aligned(16))) char lds[FS_LDS];
  const int tid = threadIdx.x, net = blockIdx.y;
  const long b0 = (long)blockIdx.x * BK_S;
  const int B = a.B;
  const Pass P = bk_pass(lds, BK_S);
  const float* x = a.x[net];
  const float* ep = a.eps[net];
  for (int i = tid; i < 16 * BK_S; i += FC_NT) {
    const int k = i / BK_S, c = i - k * BK_S;
    P.tmp[i] = (k < DD && b0 + c < B) ? x[(b0 + c) * DD + k] : 0.f;
  }
  Derivs<NH, BK_FCB> D;
  mlp_pass<DD, BK_FCB, false, ACT, NH, false, SV_SAVE>(a.f[net], nullptr, P, nullptr, &D);
  float ev[DD];
  const bool mine = tid < BK_S && b0 + tid < B;
#pragma unroll
  for (int i = 0; i < DD; ++i) ev[i] = mine ? ep[(b0 + tid) * DD + i] : 0.f;
  for (int i = tid; i < 16 * BK_S; i += FC_NT) {   // after mlp_pass's last barrier: nobody reads f(x)
    const int k = i / BK_S, c = i - k * BK_S;
    P.tmp[i] = (k < DD && b0 + c < B) ? ep[(b0 + c) * DD + k] : 0.f;
  }
  float acc = 0.f;
  for (int k = 0; k < a.n_terms; ++k) {
    mlp_pass<DD, BK_FCB, false, ACT, NH, false, SV_VJP>(a.t[net], nullptr, P, nullptr, &D);
    if (tid < BK_S) {      // rows >= DD of the VJP are zero (the transposed output planes' padding rows)
      double tr = 0.0;
#pragma unroll
      for (int i = 0; i < DD; ++i) tr += (double)P.tmp[i * BK_S + tid] * (double)ev[i];
      acc = acc + a.coeff[k] * (float)tr;
    }
  }
  if (mine) a.out[net][b0 + tid] = acc;
}

int fcseries_supported(const FcSeriesArgs& a) {
  if (a.nn < 1 || a.nn > 2 || a.B <= 0 || a.n_terms < 1 || a.n_terms > 128) return 0;
  if (!fc_block_instance(a.d, a.nl - 2, a.act)) return 0;
  for (int i = 0; i < a.nn; ++i) {
    if (!a.x[i] || !a.eps[i] || !a.out[i]) return 0;
    for (int l = 0; l < a.nl; ++l)
      if (!a.f[i].L[l].Ah || !a.f[i].L[l].Aexp || !a.t[i].L[l].Ah || !a.t[i].L[l].Aexp) return 0;
    if (!a.f[i].L[0].A || !a.t[i].L[0].A) return 0;             // the input layers' fp32 rows
  }
  return 1;
}

int launch_fcseries(const FcSeriesArgs& a, hipStream_t s) {
  if (!fcseries_supported(a)) return INF_ERR_UNSUPPORTED;
  const int nh = a.nl - 2;
  const dim3 grid((unsigned)fcblock_grid(a.B), (unsigned)a.nn);
  const bool prof = prof_enabled();
  if (prof) prof_begin_launch(s);
#define FS_GO(DD_, ACT_, NH_)                    \
  if (a.d == DD_ && a.act == ACT_ && nh == NH_) \
    hipLaunchKernelGGL((fcseries_kernel<DD_, ACT_, NH_>), grid, dim3(FC_NT), 0, s, a);
  FC_BLOCK_INSTANCES(FS_GO)
#undef FS_GO
  INF_CHECK_LAUNCH();
  if (prof) {
    // flops: the forward pass and n_terms transposed passes per sample and net
    const double f = fc_flops_per_column(a.d, a.nl) * a.B * a.nn * (1.0 + a.n_terms);
    prof_end_launch(s, 620, f, 4.0 * a.B * a.nn * (3.0 * a.d + 1.0), 3.0 * f / PEAK_BF16_FLOPS_PER_MS);
  }
  return INF_OK;
}

}  // namespace inf
