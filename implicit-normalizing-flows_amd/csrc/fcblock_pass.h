// The net passes of the device-resident fc kernels (fcblock.hip: one imBlock evaluation per launch; fcseries.inc: the
// power-series log-det per launch): a workgroup of 8 waves carries BK_S = 48 samples (or 16 samples x (d + 1) columns of
// the forward-mode Jacobian) through all layers with the activations in LDS, in fc_h3_ops.h's f16x3 arithmetic -- per
// column the bits of fcnet_h3.hip's kernels.  Maps the net evaluations inside implicit_block.py:220-260,358-362
// (nnet_x / nnet_z and batch_jacobian) and :418-426 (the series' vector-Jacobian products); the callers hold the
// algorithms around them.  Also the (d, hidden layers, activation) table both kernels are instantiated for.
#pragma once

#include <type_traits>

#include "fc_h3_ops.h"

namespace inf {

namespace {
constexpr int BK_S = 48;            // samples per workgroup
constexpr int BK_FCB = BK_S / 16;   // FWD column blocks

// the instantiations M_(d, act, hidden 128 x 128 layers) of fcblock_kernel and fcseries_kernel
#define FC_BLOCK_INSTANCES(M_) M_(6, ACT_SIN, 3) M_(6, ACT_SWISH, 3) M_(2, ACT_SIN, 1) M_(2, ACT_SWISH, 1)
inline bool fc_block_instance(int d, int nh, int act) {
#define FC_BK_IS(DD_, ACT_, NH_) \
  if (d == DD_ && act == ACT_ && nh == NH_) return true;
  FC_BLOCK_INSTANCES(FC_BK_IS)
#undef FC_BK_IS
  return false;
}

// Phase stamps (INFLOW_PHASE_STAMPS builds only, tools/build_stamps_fcblock.sh): thread 0 of every workgroup records
// s_memtime after each barrier-delimited stage; the launch prints the per-stage means.  Null buffer otherwise.
constexpr int BK_TSLOTS = 128;
struct Stamps {
  unsigned long long* buf;
  int i;
};
#if INFLOW_PHASE_STAMPS
#define BK_STAMP(T_)                                                                              \
  do {                                                                                            \
    if ((T_) && (T_)->buf && threadIdx.x == 0 && (T_)->i < BK_TSLOTS)                             \
      (T_)->buf[(long)blockIdx.x * BK_TSLOTS + (T_)->i++] = __builtin_amdgcn_s_memtime();         \
  } while (0)
#else
#define BK_STAMP(T_) \
  do {               \
    (void)(T_);      \
  } while (0)
#endif

// Workgroup barrier for LDS traffic only: waits for this wave's LDS operations, not for its global loads (the weight
// requests in flight across a layer's barriers; __syncthreads() would drain them: s_waitcnt vmcnt(0)).  Every
// intra-workgroup exchange of these kernels goes through LDS.
__device__ __forceinline__ void bk_sync() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// A net's resident weights for the solve: the hidden layers' fragments of wave w in registers; the input layer's fp32
// rows (exact VALU contraction, fcnet_common.h fc_in_col; [row][BK_W0_LD], k >= d zero) and the output layer (four k
// steps, row tile 0) as fragment planes in LDS (12 KiB at 128 wide)
template <int NH>
struct NetRegs {
  u32x4 wh[NH][4][2];
  const float* w0;   // LDS: [row * BK_W0_LD + k], row < 128, k < d
  const u32x4* wo;   // LDS: [(ks * 2 + plane) * 64 + lane], ks < 4
};
constexpr int BK_W0_LD = 8;               // floats per input-layer row in LDS (d <= 8)
constexpr int BK_W0_VEC = FC_H * BK_W0_LD / 4;   // u32x4 of the input layer's fp32 rows
constexpr int BK_WO_VEC = 4 * 2 * 64;     // u32x4 of the output layer's planes
template <int NH>
__device__ __forceinline__ void load_net(const FcArgs& a, int w, int lane, u32x4* lds_w, NetRegs<NH>& r) {
  const u32x4* go = reinterpret_cast<const u32x4*>(a.L[NH + 1].Ah);
  float* w0 = reinterpret_cast<float*>(lds_w);
  for (int i = threadIdx.x; i < FC_H * BK_W0_LD; i += FC_NT) {
    const int row = i / BK_W0_LD, k = i - row * BK_W0_LD;
    w0[i] = k < a.d ? a.L[0].A[(long)row * a.L[0].Kpad + k] : 0.f;
  }
  for (int i = threadIdx.x; i < BK_WO_VEC; i += FC_NT) lds_w[BK_W0_VEC + i] = go[i];
#pragma unroll
  for (int l = 0; l < NH; ++l) ldw_h3<4>(a.L[1 + l].Ah, 4, w, lane, r.wh[l]);
  r.w0 = w0;
  r.wo = lds_w + BK_W0_VEC;
}

// the activation derivatives a forward pass saves for the VJP passes of the power series (mlp_pass SV modes)
enum { SV_NONE = 0, SV_SAVE = 1, SV_VJP = 2 };
template <int NH, int NCB>
struct Derivs {
  float d[NH + 1][NCB][4];
};

// LDS scratch of one pass over NC columns
struct Pass {
  uint16_t* pl0;   // [col][k] h plane
  uint16_t* pl1;   // l plane
  float* tmp;      // [row][col] fp32 input rows [0, 16) / output rows [0, 16)
  float* wmax;     // [wave][col]
  int* sx;         // column scale exponents
};
__host__ __device__ inline size_t bk_al(size_t x) { return (x + 15) & ~(size_t)15; }   // (every LDS offset: 16 bytes)
__device__ __forceinline__ Pass bk_pass(char* base, int nc) {
  Pass p;
  size_t off = 0;
  p.pl0 = reinterpret_cast<uint16_t*>(base + off);
  p.pl1 = p.pl0 + (size_t)nc * FC_LD;
  off += bk_al(2 * sizeof(uint16_t) * nc * FC_LD);
  p.tmp = reinterpret_cast<float*>(base + off);
  off += bk_al(sizeof(float) * 16 * nc);
  p.wmax = reinterpret_cast<float*>(base + off);
  off += bk_al(sizeof(float) * FC_NW * nc);
  p.sx = reinterpret_cast<int*>(base + off);
  return p;
}

// One pass of the net over NC = 16 NCB columns: inputs in tmp rows [0, 16) (rows >= d zero), the output layer's sums
// (no bias) left in tmp rows [0, 16).  The arithmetic of fcnet_h3.hip per column: the input layer (K = DD) in exact fp32
// on the VALU from the fp32 rows, the others scaled two-piece fp16 operands, three products per fp32 product on
// v_mfma_f32_16x16x32_f16, fp32 accumulation, exact unscale.  JAC: column block 0 is the
// primal, the others are tangents, multiplied by act'(pre-activation of the primal).  REG: the weights come from
// registers (loaded once per solve) instead of global memory.  SV_SAVE: a forward pass that also keeps act' of
// every hidden unit in D (registers: wave w holds rows 16 w + 4 g + r of every hidden layer); SV_VJP: the pass of the
// transposed net (a.L[j] = W_{L-1-j}^T, fcseries_kernel) whose hidden epilogue is the product with D's derivatives of
// forward layer NH - j instead of bias + activation -- the row ownership of both passes is the same.
template <int DD, int NCB, bool JAC, int ACT, int NH, bool REG, int SV = SV_NONE, class NA = FcArgs>
__device__ __forceinline__ void mlp_pass(const NA& a, const NetRegs<NH>* R, const Pass& P, Stamps* ts,
                                         Derivs<NH, NCB>* D = nullptr) {
  constexpr int NC = 16 * NCB;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, g = lane >> 4;
  u32x4 wnext[4][2];
  u32x4 w0[1][2];                              // (unused: the input layer is the VALU contraction)
  float wi[4][DD];
  if constexpr (!REG) {
    fc_in_weights<DD>(a.L[0].A, a.L[0].Kpad, DD, 16 * w + 4 * g, wi);
    if (NH > 0) ldw_h3<4>(a.L[1].Ah, 4, w, lane, wnext);
  }
  bk_sync();                                   // the caller's input rows (and, REG, the resident weights)
  if constexpr (REG) fc_in_weights<DD>(R->w0, BK_W0_LD, DD, 16 * w + 4 * g, wi);
  BK_STAMP(ts);

  auto layer = [&](auto nksc, int l, const u32x4 (&wr)[decltype(nksc)::value][2]) {
    constexpr int NKS = decltype(nksc)::value;
    const FcLayer& L = a.L[l];
    float bias[4];
    if constexpr (SV != SV_VJP) {
#pragma unroll
      for (int r = 0; r < 4; ++r) bias[r] = L.b[16 * w + 4 * g + r];
    }
    const float sp = (ACT == ACT_SWISH && SV != SV_VJP) ? softplus_f(ldc(L.beta)) : 0.f;
    float v[NCB][4];
    if constexpr (NKS == 1) {
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) fc_in_col<DD>(wi, P.tmp + cb * 16 + li, NC, DD, v[cb]);
    } else {
      f32x4 acc[NCB];
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) acc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) {
          const int col = cb * 16 + li;
          const u32x4 xh = *reinterpret_cast<const u32x4*>(P.pl0 + col * FC_LD + ks * 32 + 8 * g);
          const u32x4 xl = *reinterpret_cast<const u32x4*>(P.pl1 + col * FC_LD + ks * 32 + 8 * g);
          acc[cb] = mfma3(wr[ks], xh, xl, acc[cb]);
        }
      const int sw = ldc(L.Aexp);
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) {
        const int e = -(sw + P.sx[cb * 16 + li]);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[cb][r] = __builtin_amdgcn_ldexpf(acc[cb][r], e);
      }
    }
    constexpr int EP = SV == SV_VJP ? EP_VJP : (SV == SV_SAVE ? EP_SAVE : (JAC ? EP_JAC : EP_ACT));
    if constexpr (SV == SV_NONE) h3_epilogue<EP, ACT, NCB>(v, [&](int r) { return bias[r]; }, sp);
    else h3_epilogue<EP, ACT, NCB>(v, [&](int r) { return bias[r]; }, sp, D->d[SV == SV_VJP ? NH - l : l]);
    // Sin nets: the fixed scales of fcnet_h3.hip (the forward and primal values in [-1/(2 pi), 1/(2 pi)], the tangents
    // bounded by the Lipschitz caps where every coeff <= 1) -- no column-max exchange; else per-column maxima.  (The
    // transposed passes of the series keep per-column scales: their vectors carry the probe's norm.)
    bool allfix = false;
    if constexpr (ACT == ACT_SIN && SV != SV_VJP) {
      if constexpr (JAC) allfix = a.tan_fixed != 0;
      else allfix = true;
    }
    if (allfix) {
      bk_sync();                                 // every wave is done reading this layer's input planes
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) {
        const int col = cb * 16 + li;
        const int e = (JAC && cb > 0) ? FC_SFIXT : FC_SFIX;
        uint2 h, lo;
        split4(v[cb], __builtin_amdgcn_ldexpf(1.f, e), h, lo);
        *reinterpret_cast<uint2*>(P.pl0 + col * FC_LD + 16 * w + 4 * g) = h;
        *reinterpret_cast<uint2*>(P.pl1 + col * FC_LD + 16 * w + 4 * g) = lo;
        if (w == 0 && g == 0) P.sx[col] = e;
      }
    } else {
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) {
        float m = fmaxf(fmaxf(fabsf(v[cb][0]), fabsf(v[cb][1])), fmaxf(fabsf(v[cb][2]), fabsf(v[cb][3])));
        m = fmaxf(m, __shfl_xor(m, 16, 64));
        m = fmaxf(m, __shfl_xor(m, 32, 64));
        if (g == 0) P.wmax[w * NC + cb * 16 + li] = m;
      }
      bk_sync();
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) {
        const int col = cb * 16 + li;
        float m = 0.f;
#pragma unroll
        for (int ww = 0; ww < FC_NW; ++ww) m = fmaxf(m, P.wmax[ww * NC + col]);
        const int e = (ACT == ACT_SIN && SV != SV_VJP && cb == 0) ? FC_SFIX : h3_scale_exp(m);
        uint2 h, lo;
        split4(v[cb], __builtin_amdgcn_ldexpf(1.f, e), h, lo);
        *reinterpret_cast<uint2*>(P.pl0 + col * FC_LD + 16 * w + 4 * g) = h;
        *reinterpret_cast<uint2*>(P.pl1 + col * FC_LD + 16 * w + 4 * g) = lo;
        if (w == 0 && g == 0) P.sx[col] = e;
      }
    }
    bk_sync();
    BK_STAMP(ts);
  };
  if constexpr (REG) {
    layer(std::integral_constant<int, 1>(), 0, w0);
#pragma unroll
    for (int l = 0; l < NH; ++l) layer(std::integral_constant<int, 4>(), 1 + l, R->wh[l]);
  } else {
    layer(std::integral_constant<int, 1>(), 0, w0);
#pragma unroll
    for (int l = 0; l < NH; ++l) {
      u32x4 wc[4][2];
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        wc[ks][0] = wnext[ks][0];
        wc[ks][1] = wnext[ks][1];
      }
      if (l + 1 < NH) ldw_h3<4>(a.L[2 + l].Ah, 4, w, lane, wnext);
      layer(std::integral_constant<int, 4>(), 1 + l, wc);
    }
  }
  // output layer: 16 padded rows (d valid), K = 128; column block w on wave w
  if (w < NCB) {
    const FcLayer& L = a.L[NH + 1];
    u32x4 wo[4][2];
    if constexpr (REG) {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        wo[ks][0] = R->wo[(ks * 2 + 0) * 64 + lane];
        wo[ks][1] = R->wo[(ks * 2 + 1) * 64 + lane];
      }
    } else {
      ldw_h3<4>(L.Ah, 4, 0, lane, wo);
    }
    const int col = w * 16 + li;
    h3_out_layer<FC_LD>(wo, L.Aexp, P.pl0, P.pl1, col, g, [&]() { return P.sx[col]; }, P.tmp, NC);
  }
  bk_sync();
  BK_STAMP(ts);
}

// The forward-mode Jacobian pass (JAC of mlp_pass) with half the LDS operand traffic: the 8 waves form 4 row groups of
// 32 rows (two 16-row tiles each, both fed by every B fragment read) x 2 column groups; column group c takes the primal
// column block 0 and tangent blocks [1 + c NT / 2, 1 + (c + 1) NT / 2) (the primal is computed by both groups: each
// needs act' of its rows).  The arithmetic per column is mlp_pass's (same products, same order, same scales); weights
// stream from global memory, each layer's requested right after the previous layer's products.
template <int DD, int NCB, int ACT, int NH>
__device__ __forceinline__ void mlp_jac2(const FcArgs& a, const Pass& P, Stamps* ts) {
  constexpr int NC = 16 * NCB;
  constexpr int NT = NCB - 1;                 // tangent blocks (even)
  constexpr int NJ = 1 + NT / 2;              // column blocks per wave
  static_assert(NT % 2 == 0, "even tangent count");
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, g = lane >> 4;
  const int rg = w & 3, cg = w >> 2;
  auto cbof = [&](int j) { return j == 0 ? 0 : j + cg * (NT / 2); };
  u32x4 wi[2][1][2];                           // (unused: the input layer is the VALU contraction)
  float wf[2][4][DD];
  fc_in_weights<DD>(a.L[0].A, a.L[0].Kpad, DD, 16 * (2 * rg + 0) + 4 * g, wf[0]);
  fc_in_weights<DD>(a.L[0].A, a.L[0].Kpad, DD, 16 * (2 * rg + 1) + 4 * g, wf[1]);
  u32x4 wh[2][4][2];
  if (NH > 0) {
    ldw_h3<4>(a.L[1].Ah, 4, 2 * rg + 0, lane, wh[0]);
    ldw_h3<4>(a.L[1].Ah, 4, 2 * rg + 1, lane, wh[1]);
  }
  bk_sync();                                   // the caller's input rows
  BK_STAMP(ts);
  auto layer = [&](auto nksc, int l, u32x4 (&wr)[2][decltype(nksc)::value][2]) {
    constexpr int NKS = decltype(nksc)::value;
    const FcLayer& L = a.L[l];
    const float sp = (ACT == ACT_SWISH) ? softplus_f(ldc(L.beta)) : 0.f;
    float v[2][NJ][4];
    if constexpr (NKS == 1) {
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int j = 0; j < NJ; ++j) fc_in_col<DD>(wf[t], P.tmp + cbof(j) * 16 + li, NC, DD, v[t][j]);
    } else {
      f32x4 acc[2][NJ];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[t][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const int col = cbof(j) * 16 + li;
          const u32x4 xh = *reinterpret_cast<const u32x4*>(P.pl0 + col * FC_LD + ks * 32 + 8 * g);
          const u32x4 xl = *reinterpret_cast<const u32x4*>(P.pl1 + col * FC_LD + ks * 32 + 8 * g);
          acc[0][j] = mfma3(wr[0][ks], xh, xl, acc[0][j]);
          acc[1][j] = mfma3(wr[1][ks], xh, xl, acc[1][j]);
        }
      // the next hidden layer's weights, in flight during this epilogue
      if (l + 1 <= NH) {
        ldw_h3<4>(a.L[l + 1].Ah, 4, 2 * rg + 0, lane, wh[0]);
        ldw_h3<4>(a.L[l + 1].Ah, 4, 2 * rg + 1, lane, wh[1]);
      }
      const int sw = ldc(L.Aexp);
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int e = -(sw + P.sx[cbof(j) * 16 + li]);
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) v[t][j][r] = __builtin_amdgcn_ldexpf(acc[t][j][r], e);
      }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t)
      h3_epilogue<EP_JAC, ACT, NJ>(v[t], [&](int r) { return L.b[16 * (2 * rg + t) + 4 * g + r]; }, sp);
    const bool allfix = ACT == ACT_SIN && a.tan_fixed;   // (mlp_pass's fixed scales)
    if (!allfix) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        float m = 0.f;
#pragma unroll
        for (int t = 0; t < 2; ++t)
          m = fmaxf(m, fmaxf(fmaxf(fabsf(v[t][j][0]), fabsf(v[t][j][1])), fmaxf(fabsf(v[t][j][2]), fabsf(v[t][j][3]))));
        m = fmaxf(m, __shfl_xor(m, 16, 64));
        m = fmaxf(m, __shfl_xor(m, 32, 64));
        if (g == 0 && (j > 0 || cg == 0)) P.wmax[rg * NC + cbof(j) * 16 + li] = m;
      }
    }
    bk_sync();
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      if (j == 0 && cg != 0) continue;           // the primal's planes come from column group 0
      const int col = cbof(j) * 16 + li;
      int e;
      if (allfix) {
        e = j == 0 ? FC_SFIX : FC_SFIXT;
      } else {
        const float m = fmaxf(fmaxf(P.wmax[0 * NC + col], P.wmax[1 * NC + col]),
                              fmaxf(P.wmax[2 * NC + col], P.wmax[3 * NC + col]));
        e = (ACT == ACT_SIN && j == 0) ? FC_SFIX : h3_scale_exp(m);
      }
      const float S2 = __builtin_amdgcn_ldexpf(1.f, e);
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        uint2 h, lo;
        split4(v[t][j], S2, h, lo);
        *reinterpret_cast<uint2*>(P.pl0 + col * FC_LD + 16 * (2 * rg + t) + 4 * g) = h;
        *reinterpret_cast<uint2*>(P.pl1 + col * FC_LD + 16 * (2 * rg + t) + 4 * g) = lo;
      }
      if (rg == 0 && g == 0) P.sx[col] = e;
    }
    bk_sync();
    BK_STAMP(ts);
  };
  layer(std::integral_constant<int, 1>(), 0, wi);
#pragma unroll
  for (int l = 0; l < NH; ++l) layer(std::integral_constant<int, 4>(), 1 + l, wh);
  // output layer: 16 padded rows (d valid), K = 128; column block w on wave w
  if (w < NCB) {
    const FcLayer& L = a.L[NH + 1];
    u32x4 wo[4][2];
    ldw_h3<4>(L.Ah, 4, 0, lane, wo);
    const int col = w * 16 + li;
    h3_out_layer<FC_LD>(wo, L.Aexp, P.pl0, P.pl1, col, g, [&]() { return P.sx[col]; }, P.tmp, NC);
  }
  bk_sync();
  BK_STAMP(ts);
}
}  // namespace

}  // namespace inf
