// The per-element arithmetic that the output stage (out_stage.hip), the Broyden kernels (broyden.hip) and the fused fc
// nets' epilogues (fcnet.hip, fcnet_h3.hip) share.  Several of these are rounding contracts with the reference (the
// order of two fp32 operations), and every kernel that forms one must form the same bits: each is defined here once.
#pragma once
#include "kernels.h"

namespace inf {

constexpr int OUT_CH = 1024;   // elements per block of the output stage: one per thread (4 per thread of 256 was
                               // latency-bound, 19 us per CIFAR residual at B=64)
constexpr int SS_MAXCH = 4;    // most chunks per sample a one-block-per-sample residual kernel sums (OutArgs::sample_sums)
// the wide fc output stage's internal mode beside the OutModes: the implicit backward's residual
constexpr int OM_WIDE_VJPRES = 5;

// ---- the output stage's values (implicit_block.py:60,72,227,186-190) -------------------------------------------------
// x_embed = nnet_x(x) + x
__device__ __forceinline__ float embed_value(float v, float x) { return v + x; }
// the Broyden residual g(z) = (x_embed - nnet_z(z)) - z
__device__ __forceinline__ float resid_value(float xemb, float v, float z) { return (xemb - v) - z; }
// the recompute z = (nnet_x(x) - nnet_z(z*)) + x
__device__ __forceinline__ float recomp_value(float fx, float v, float x) { return (fx - v) + x; }
// the implicit backward's residual g(y) = (y + y^T J) - grad
__device__ __forceinline__ float vjp_resid_value(float y, float v, float grad) { return (y + v) - grad; }
// OM_VJP of preact nets: v times the leading activation's derivative at x_in = in1 (swish' with sp = softplus(beta), or
// a parameter-less kind)
__device__ __forceinline__ float vjp_factor(const OutArgs& a, float v, long ei, float sp) {
  if (a.pre_beta) v = v * swish_d(a.in1[ei], sp);
  else if (a.pre_act != ACT_NONE) v = v * act_any_d(a.pre_act, a.in1[ei]);
  return v;
}

// One element of the output stage: s the last layer's sum at feature c, ei its element index; `mode` an OutMode or
// OM_WIDE_VJPRES (kernels.h OutArgs lists what each reads and writes), acc the thread's fp64 partial (g^2 or v.eps).
// WIDE (fc_out_wide_kernel, mode a compile-time constant there): OM_RESID's bias may be null (the broadcast f(0) has it).
template <bool WIDE = false>
__device__ __forceinline__ void out_epilogue(const OutArgs& a, int mode, float s, int c, long ei, float sp, double& acc) {
  switch (mode) {
    case OM_PLAIN: a.out0[ei] = s + a.bias[c]; break;
    case OM_EMBED: {
      const float v = s + a.bias[c];
      a.out0[ei] = v;
      a.out1[ei] = embed_value(v, a.in0[ei]);
      break;
    }
    case OM_RESID: {
      const float v = (!WIDE || a.bias) ? s + a.bias[c] : s;
      const float gx = resid_value(a.in0[ei], v, a.in1[ei]);
      a.out0[ei] = gx;
      if (a.in2) a.out1[ei] = gx - a.in2[ei];
      if (a.out2) a.out2[ei] = v;
      acc += (double)gx * (double)gx;
      break;
    }
    case OM_RECOMP: a.out0[ei] = recomp_value(a.in0[ei], s + a.bias[c], a.in1[ei]); break;
    default:
      if (!WIDE || mode == OM_VJP) {
        const float v = vjp_factor(a, s, ei, sp);
        a.out0[ei] = v;
        if (a.partial) acc += (double)v * (double)a.in0[ei];
      } else {   // OM_WIDE_VJPRES
        const float gv = vjp_resid_value(a.in0[ei], s, a.in1[ei]);
        a.out0[ei] = gv;
        if (a.in2) a.out1[ei] = gv - a.in2[ei];
        acc += (double)gv * (double)gv;
      }
  }
}

// The per-sample total of a one-block-per-sample kernel: the block sums of its NCH chunks added in chunk order from 0.0,
// as the chunked kernels' partials are by reduce_partials_kernel -- the same bits without the reduction launch.
template <int NCH>
__device__ __forceinline__ double sample_total(const double* acc, double* red) {
  double tot = 0.0;
#pragma unroll
  for (int cc = 0; cc < NCH; ++cc) tot += block_sum(acc[cc], red);
  return tot;
}

// ---- Broyden (broyden.py:94-99,153,177-178) --------------------------------------------------------------------------
// x_est = x0 + update; delta_x = x_est - x0 (xe and dx may be stores)
__device__ __forceinline__ void broyden_step(float x0, float up, float& xe, float& dx) {
  const float e = x0 + up;
  xe = e;
  dx = e - x0;
}
// element i of sample b
__device__ __forceinline__ long br_idx(const BroydenArgs& a, int b, int i) { return (long)b * a.sb + (long)i * a.si; }
// per-sample rule: a stopped sample keeps its iterate (and its U / VT columns)
__device__ __forceinline__ void keep_iterate(const BroydenArgs& a, long e) {
  a.xnew[e] = a.x[e];
  a.dxnew[e] = 0.f;
  a.upd[e] = 0.f;
}
// the update's stores: update, x_new = x + update, dx_new = x_new - x
__device__ __forceinline__ void store_update(const BroydenArgs& a, long e, float up) {
  a.upd[e] = up;
  broyden_step(a.x[e], up, a.xnew[e], a.dxnew[e]);
}
// NaN -> 0 in the new column's vT and u
__device__ __forceinline__ void scrub_nan(float& vt, float& u) {
  if (vt != vt) vt = 0.f;
  if (u != u) u = 0.f;
}

}  // namespace inf
