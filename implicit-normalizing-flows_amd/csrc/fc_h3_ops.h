// The scaled two-piece fp16 ("f16x3", common.h) arithmetic that the fused fc kernels share, defined once: fcnet_h3.hip
// (fcnet_h3_body) and the block / series kernels' passes (fcblock_pass.h mlp_pass, mlp_jac2) call these and are required
// to form the same bits per column (tests/test_gpu_fc_fused_bits.py).  fcnet_h3.hip's header explains the operand layout
// and the scales.  Here: the three-product MFMA step, the weight fragment loader, the split, the hidden epilogue by
// mode and the 16-row output layer.  A layer's product loop, its exact unscale and the column-scale exchange with the
// plane store stay written out in each kernel: shared, they moved the block kernel's machine code.
#pragma once

#include "fcnet_common.h"

namespace inf {

constexpr int FC_NW = 8;             // waves per workgroup of the f16x3 fc kernels: wave w owns rows [16 w, 16 w + 16)
constexpr int FC_NT = 64 * FC_NW;
constexpr int FC_LD = FC_H + 8;      // halves per activation-plane column (272 B: 16-byte aligned, spreads the banks)

__device__ __forceinline__ f32x4 mfma3(const u32x4 (&a)[2], const u32x4& xh, const u32x4& xl, f32x4 c) {
  const f16x8 ah = __builtin_bit_cast(f16x8, a[0]), al = __builtin_bit_cast(f16x8, a[1]);
  const f16x8 bh = __builtin_bit_cast(f16x8, xh), bl = __builtin_bit_cast(f16x8, xl);
  c = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh, c, 0, 0, 0);
  return c;
}

// the (h, l) fragments of row tile rt, k steps [0, NKS), of a layer's planes (fragment tile (rt nks + ks): 2 x 512 halves)
template <int NKS>
__device__ __forceinline__ void ldw_h3(const uint16_t* A, int nks, int rt, int lane, u32x4 (&w)[NKS][2]) {
  const u32x4* p = reinterpret_cast<const u32x4*>(A);
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    const long t = (long)rt * nks + ks;
    w[ks][0] = p[(t * 2 + 0) * 64 + lane];
    w[ks][1] = p[(t * 2 + 1) * 64 + lane];
  }
}

// 4 fp32 values (consecutive rows of one column) -> scaled fp16 h / l pieces, packed
__device__ __forceinline__ void split4(const float (&v)[4], float S, uint2& h, uint2& l) {
  _Float16 hh[4], ll[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    hh[r] = (_Float16)(v[r] * S);
    ll[r] = (_Float16)__builtin_fmaf(v[r], S, -(float)hh[r]);
  }
  const f16x2 a = {hh[0], hh[1]}, b = {hh[2], hh[3]}, c = {ll[0], ll[1]}, e = {ll[2], ll[3]};
  h = make_uint2(__builtin_bit_cast(unsigned, a), __builtin_bit_cast(unsigned, b));
  l = make_uint2(__builtin_bit_cast(unsigned, c), __builtin_bit_cast(unsigned, e));
}

// ---- the hidden epilogue of one row tile (bias: the lane's 4 rows).  EP_ACT: bias + activation; EP_JAC: column block
// 0 is the primal, the others are tangents times act'(the primal's pre-activation); EP_SAVE: EP_ACT that also keeps
// act' in dv; EP_VJP: the transposed pass, times the saved derivatives dv
enum { EP_ACT = 0, EP_JAC = 1, EP_SAVE = 2, EP_VJP = 3 };
template <int EP, int ACT, int NCB, class Bias>
__device__ __forceinline__ void h3_epilogue(float (&v)[NCB][4], Bias bias, float sp, float (*dv)[4] = nullptr) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if constexpr (EP == EP_VJP) {
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) v[cb][r] *= dv[cb][r];
    } else if constexpr (EP == EP_SAVE) {
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) fc_act_fd<ACT>(v[cb][r] + bias(r), sp, v[cb][r], dv[cb][r]);
    } else if constexpr (EP == EP_JAC) {
      const float z = v[0][r] + bias(r);
      float dd;
      fc_act_fd<ACT>(z, sp, v[0][r], dd);
#pragma unroll
      for (int cb = 1; cb < NCB; ++cb) v[cb][r] *= dd;
    } else {
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) v[cb][r] = fc_act_f<ACT>(v[cb][r] + bias(r), sp);
    }
  }
}

// ---- the output layer: 16 padded rows (d valid), K = 128 (wo: row tile 0's four k steps), of plane column col, whose
// planes have LD halves per column; the fp32 sums (no bias) go to tmp[row][col] (row stride NC), unscaled exactly by
// -(*aexp + sx()), sx() the column's scale exponent
template <int LD, class Sx>
__device__ __forceinline__ void h3_out_layer(const u32x4 (&wo)[4][2], const int* aexp, const uint16_t* ph,
                                             const uint16_t* pl, int col, int g, Sx sx, float* tmp, int NC) {
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    const u32x4 xh = *reinterpret_cast<const u32x4*>(ph + col * LD + ks * 32 + 8 * g);
    const u32x4 xl = *reinterpret_cast<const u32x4*>(pl + col * LD + ks * 32 + 8 * g);
    acc = mfma3(wo[ks], xh, xl, acc);
  }
  const int e = -(ldc(aexp) + sx());
#pragma unroll
  for (int r = 0; r < 4; ++r) tmp[(4 * g + r) * NC + col] = __builtin_amdgcn_ldexpf(acc[r], e);
}

}  // namespace inf
