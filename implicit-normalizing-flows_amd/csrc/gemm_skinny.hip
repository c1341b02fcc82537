// Skinny GEMMs of wide fc nets: the per-layer contraction of gemm.hip,
//   out[m][n] = epi( sum_k A[m][k] * X'[k][n] ),   X' = pre(X),  feature-major (rows, B) tensors (P = N = B, x_sample = 0),
// at the shapes a (d, B) net has: few columns (N = B = 64), one very deep or very tall layer (d -> hidden, hidden -> d)
// and small square ones.  gemm.hip's 128 x 128 tile gives these 1 - 24 workgroups on a 256-CU part.  Two forms:
//
//   * small tile: one wave per 32 x 32 MFMA tile, workgroups of 1 x 1, 1 x 2 or 2 x 2 waves (32 x 32 .. 64 x 64 outputs),
//     the epilogue in the kernel;
//   * split K: the same kernel over a grid (M tiles) x (N tiles) x (S slices of K); a workgroup contracts its slice and
//     stores the fp32 partial tile into slab[s][m][n]; a second launch sums the S partials of an element in slice order
//     in fp64, rounds once and applies the epilogue.  No atomics: the result does not depend on scheduling.
//
// Arithmetic is the exact fp32 MFMA (v_mfma_f32_32x32x2_f32) whatever the net's INF_MFMA_* mode: these shapes are bound
// by latency and by the operand stream, not by the matrix pipe.  The LDS images and the k-permutation are gemm.hip's
// (A rows at a 20-float pitch read as two ds_read_b128, B as [k][n] read one ds_read_b32 per MFMA step, both
// conflict-free), four 16-deep sub-tiles side by side per 64-deep K tile (A pitch 68: the same bank pattern).  With a
// handful of MFMAs per wave and K tile nothing hides a global load, so a launch costs one load round trip per K tile:
// the 64-deep tile makes that a quarter of what 16-deep tiles cost (measured).  Register-staged double
// buffering, one barrier per K tile.  The MFMA sequence of an output element is gemm.hip's f32 mode's (k ascending in
// steps of 16, the same lane permutation), so an unsplit layer gives the bits launch_gemm gives in INF_MFMA_F32.
// X is loaded one float per lane (lanes along n: coalesced), so any N, any alignment of X and N = 1 take the same path.
#include "kernels.h"

namespace inf {

namespace {

constexpr int SK_CUS = 256;        // MI355X compute units: the grid size a launch wants to reach
constexpr int SK_DEEP_K = 256;     // split K from here on: four slices of the minimum depth
constexpr int SK_BK = 64;          // K tile; slices are whole K tiles, so this is also the minimum K per slice

// The epilogues fc nets reach, written once for the small-tile kernel and the split-K reduce.  `epi` is uniform over the
// launch; o = m * P + n.  (EP_BIAS_ACT arrives resolved to EP_ACT_*; a bias-free layer's bias is the engine's zero vector.)
// The element's second operand -- the EP_MUL_DERIV multiplier, else the bias -- comes from skinny_aux: the tile kernel
// loads its 16 before the K loop, so that its epilogue is stores only (a load between two stores costs a full wait each).
__device__ __forceinline__ float skinny_aux(const GemmArgs& g, int epi, int m, long o) {
  return epi == EP_MUL_DERIV ? g.deriv_in[o] : (epi == EP_STORE ? 0.f : g.bias[m]);
}
__device__ __forceinline__ void skinny_epilogue(const GemmArgs& g, int epi, float act_sp, float v, float aux, long o) {
  switch (epi) {
    case EP_STORE: g.out[o] = v; break;
    case EP_BIAS: g.out[o] = v + aux; break;
    case EP_MUL_DERIV: g.out[o] = v * aux; break;
    default: {
      const float z = v + aux;
      float f, d;
      if (epi == EP_ACT_SWISH) {
        f = swish_f(z, act_sp);
        d = swish_d(z, act_sp);
      } else if (epi == EP_ACT_SIN) {
        f = sinact_f(z);
        d = sinact_d(z);
      } else if (epi == EP_ACT_ANY) {
        f = act_any_f(g.act, z);
        d = act_any_d(g.act, z);
      } else {
        f = z;
        d = 1.f;
      }
      if (g.deriv_out) g.deriv_out[o] = d;
      if (g.write_out) g.out[o] = f;
    }
  }
}

// the loader-side leading activation (launch_gemm_skinny admitted the combination)
__device__ __forceinline__ float skinny_pre(const GemmArgs& g, float pre_sp, float v) {
  if (g.pre_beta) return swish_f(v, pre_sp);
  if (g.pre_act == ACT_SIN) return sinact_f(v);
  return act_any_f(g.pre_act, v);
}

// Workgroup (mt, nt, slice): K tiles [slice * tps, min(nk, (slice + 1) * tps)) of SK_BK (the last one may be ragged:
// Kpad is a multiple of 16; A columns from Kpad on and X rows from Ktot on are taken as zero, not read).  SPLIT: the raw partial goes to
// slab[(slice * rows + m) * N + n], rows = M tiles * BM; else S = 1 and the epilogue runs here.
template <int WM, int WN, bool SPLIT>
__global__ __launch_bounds__(WM* WN * 64) void gemm_skinny_kernel(GemmArgs g, int epi, int tps, float* slab) {
  constexpr int NT = WM * WN * 64;
  constexpr int BM = WM * 32;
  constexpr int BN = WN * 32;
  constexpr int BK = SK_BK;
  constexpr int LDA = BK + 4;
  constexpr int A_F4 = BM * BK / 4;
  constexpr int A_PER = A_F4 / NT;
  constexpr int B_PER = BK * BN / NT;
  constexpr int KSTEP = NT / BN;
  static_assert(A_F4 % NT == 0 && (BK * BN) % NT == 0 && NT % BN == 0, "tile");

  __shared__ __attribute__((aligned(16))) float As[2][BM * LDA];
  __shared__ __attribute__((aligned(16))) float Bs[2][BK * BN];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid % WN;
  const int li = lane & 31, lh = lane >> 5;

  const int nMt = (g.M + BM - 1) / BM;
  const int nNt = (g.N + BN - 1) / BN;
  int bid = blockIdx.x;
  const int mt = bid % nMt;
  bid /= nMt;
  const int nt = bid % nNt;
  const int slice = bid / nNt;
  const int m0 = mt * BM, n0 = nt * BN;
  const int nk = (g.Kpad + BK - 1) / BK;
  const int kt0 = slice * tps;
  const int kt1 = min(nk, kt0 + tps);

  const float pre_sp = g.pre_beta ? softplus_f(*g.pre_beta) : 0.f;

  // B loader: the thread owns column j of the tile, rows kr0 + i * KSTEP of every K tile
  const int j = tid % BN;
  const int kr0 = tid / BN;
  const bool colok = n0 + j < g.N;
  const float* colbase = g.X + (colok ? n0 + j : 0);
  const bool has_pre = g.pre_beta || g.pre_act != ACT_NONE;

  f32x4 ra[A_PER];
  float rb[B_PER];

  auto load_tile = [&](int k0) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < A_PER; ++i) {
      const int f = tid + i * NT;
      const int row = f / (BK / 4), c4 = f % (BK / 4);
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (k0 + c4 * 4 < g.Kpad) v = *reinterpret_cast<const f32x4*>(g.A + (long)(m0 + row) * g.Kpad + k0 + c4 * 4);
      ra[i] = v;
    }
    // every load is issued before any is used: the address is clamped into X (row Ktot - 1, column 0) instead of
    // branching round the load, and what was clamped is zeroed afterwards
#pragma unroll
    for (int i = 0; i < B_PER; ++i) rb[i] = colbase[(long)min(k0 + kr0 + i * KSTEP, g.Ktot - 1) * g.P];
    if (has_pre) {
#pragma unroll
      for (int i = 0; i < B_PER; ++i) rb[i] = skinny_pre(g, pre_sp, rb[i]);
    }
#pragma unroll
    for (int i = 0; i < B_PER; ++i) rb[i] = (colok && k0 + kr0 + i * KSTEP < g.Ktot) ? rb[i] : 0.f;
  };
  auto store_tile = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < A_PER; ++i) {
      const int f = tid + i * NT;
      const int row = f / (BK / 4), c4 = f % (BK / 4);
      *reinterpret_cast<f32x4*>(&As[buf][row * LDA + c4 * 4]) = ra[i];
    }
#pragma unroll
    for (int i = 0; i < B_PER; ++i) Bs[buf][(kr0 + i * KSTEP) * BN + j] = rb[i];
  };

  // C/D map of the 32x32 f32 MFMA: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
  const int n = n0 + wn * 32 + li;
  const int mrow0 = m0 + wm * 32 + 4 * lh;
  float aux[SPLIT ? 1 : 16];
  if constexpr (!SPLIT) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = mrow0 + (r & 3) + 8 * (r >> 2);
      aux[r] = (n < g.N && m < g.M) ? skinny_aux(g, epi, m, (long)m * g.P + n) : 0.f;
    }
  }

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  if (kt0 < kt1) {
    load_tile(kt0 * BK);
    store_tile(0);
  }
  __syncthreads();
  for (int kt = kt0; kt < kt1; ++kt) {
    const int cur = (kt - kt0) & 1;
    if (kt + 1 < kt1) load_tile((kt + 1) * BK);
#pragma unroll
    for (int sub = 0; sub < BK / 16; ++sub) {   // lane half lh takes k = sub * 16 + lh * 8 + kk at MFMA step kk
      const float* src = &As[cur][(wm * 32 + li) * LDA + sub * 16 + lh * 8];
      const f32x4 v0 = *reinterpret_cast<const f32x4*>(src);
      const f32x4 v1 = *reinterpret_cast<const f32x4*>(src + 4);
      const float af[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
      for (int kk = 0; kk < 8; ++kk) {
        const float bf = Bs[cur][(sub * 16 + lh * 8 + kk) * BN + wn * 32 + li];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[kk], bf, acc, 0, 0, 0);
      }
    }
    if (kt + 1 < kt1) {
      store_tile(cur ^ 1);
      __syncthreads();
    }
  }

  if (n >= g.N) return;
  if constexpr (SPLIT) {
    const long rows = (long)nMt * BM;
    float* dst = slab + ((long)slice * rows) * g.N + n;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = mrow0 + (r & 3) + 8 * (r >> 2);
      if (m < g.M) dst[(long)m * g.N] = acc[r];
    }
  } else {
    const float act_sp = epi == EP_ACT_SWISH ? softplus_f(*g.act_beta) : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = mrow0 + (r & 3) + 8 * (r >> 2);
      if (m < g.M) skinny_epilogue(g, epi, act_sp, acc[r], aux[r], (long)m * g.P + n);
    }
  }
}

// out[m][n] = epi( fl32( sum_s slab[(s * rows + m) * N + n] in fp64, s ascending ) ), one thread per element
__global__ __launch_bounds__(256) void gemm_skinny_reduce_kernel(GemmArgs g, int epi, int S, long rows,
                                                                 const float* slab) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)g.M * g.N) return;
  const int m = (int)(idx / g.N);
  const int n = (int)(idx - (long)m * g.N);
  const float* src = slab + (long)m * g.N + n;
  const long stride = rows * g.N;
  double sum = 0.0;
  for (int s = 0; s < S; ++s) sum += (double)src[s * stride];
  const float act_sp = epi == EP_ACT_SWISH ? softplus_f(*g.act_beta) : 0.f;
  skinny_epilogue(g, epi, act_sp, (float)sum, skinny_aux(g, epi, m, idx), idx);
}

template <int WM, int WN>
int run_tile(const GemmArgs& g, int epi, int S, int tps, float* slab, hipStream_t s) {
  constexpr int BM = WM * 32, BN = WN * 32;
  const long nb = (long)((g.M + BM - 1) / BM) * ((g.N + BN - 1) / BN) * S;
  if (nb > 0x7fffffffL) return INF_ERR_INVALID;
  const bool prof = prof_enabled();
  if (prof) prof_begin_launch(s);
  if constexpr (WM == 1 && WN == 1) {   // (only the 32 x 32 tile is ever split: see launch_gemm_skinny)
    if (S > 1)
      hipLaunchKernelGGL((gemm_skinny_kernel<1, 1, true>), dim3((unsigned)nb), dim3(64), 0, s, g, epi, tps, slab);
    else
      hipLaunchKernelGGL((gemm_skinny_kernel<1, 1, false>), dim3((unsigned)nb), dim3(64), 0, s, g, epi, tps, slab);
  } else {
    if (S > 1) return INF_ERR_INVALID;
    hipLaunchKernelGGL((gemm_skinny_kernel<WM, WN, false>), dim3((unsigned)nb), dim3(WM * WN * 64), 0, s, g, epi, tps,
                       slab);
  }
  INF_CHECK_LAUNCH();
  if (prof) {
    // algorithmic work as gemm.hip run<>: 2 M N K flops; bytes = A + B operand + output (+ deriv), or the S partial tiles
    const double flops = 2.0 * g.M * (double)g.N * g.Ktot;
    const bool dio = epi == EP_MUL_DERIV || (epi >= EP_ACT_SWISH && g.deriv_out);
    const double outw = S > 1 ? (double)S : 1.0 + (dio ? 1.0 : 0.0);
    const double bytes = 4.0 * ((double)g.M * g.Ktot + (double)g.Ktot * g.N + (double)g.M * g.N * outw);
    prof_end_launch(s, S > 1 ? 960 : 962, flops, bytes, flops / PEAK_F32_FLOPS_PER_MS);
  }
  return INF_OK;
}

}  // namespace

// Split-K slices for the shape, 1: the small-tile form.  Split when even 32 x 32 tiles leave CUs idle and K is deep; S as
// many slices as the slab holds (rows of whole 64-row tiles), each a whole number of SK_BK-deep K tiles.
int gemm_skinny_slices(int M, int N, int Ktot, int Kpad, size_t slab_bytes, int* tps_out) {
  const int nk = (Kpad + SK_BK - 1) / SK_BK;
  int S = 1;
  const long t32 = (long)((M + 31) / 32) * ((N + 31) / 32);
  if (t32 < SK_CUS && Ktot >= SK_DEEP_K && N > 0) {
    const size_t per = (size_t)((M + 63) / 64 * 64) * (size_t)N * sizeof(float);
    const size_t fit = slab_bytes / per;
    S = (int)std::min<size_t>(fit, (size_t)(Ktot / SK_BK));
    if (S < 2) S = 1;
  }
  const int tps = (nk + S - 1) / S;
  S = (nk + tps - 1) / tps;   // no empty slice: the reduce reads S partials, every one written by this call
  if (tps_out) *tps_out = tps;
  return S;
}

int launch_gemm_skinny(const GemmArgs& g, int epi, float* slab, size_t slab_bytes, hipStream_t s) {
  if (epi == EP_BIAS_ACT)
    epi = g.act == ACT_SWISH ? EP_ACT_SWISH
                             : (g.act == ACT_SIN ? EP_ACT_SIN : (g.act == ACT_NONE ? EP_ACT_NONE : EP_ACT_ANY));
  if (epi == EP_BIAS_PRIMAL || epi < 0 || epi > EP_ACT_ANY) return INF_ERR_INVALID;
  // the leading activation under launch_gemm's rule: a Swish comes with its beta, a parameter-less one in front of an
  // EP_ACT_ANY layer, a Sin in front of a Sin layer
  if (!g.pre_beta && g.pre_act == ACT_SWISH) return INF_ERR_INVALID;
  if (!g.pre_beta && g.pre_act != ACT_NONE && !(g.pre_act == ACT_SIN ? epi == EP_ACT_SIN : epi == EP_ACT_ANY))
    return INF_ERR_UNSUPPORTED;
  if (g.Kpad % 16 != 0 || g.M <= 0 || g.Ktot <= 0 || g.Ktot > g.Kpad || g.N < 0 || g.P != g.N || g.x_sample != 0 || g.o_sample != 0) return INF_ERR_INVALID;
  if (g.N == 0) return INF_OK;
  int tps = 0;
  const int S = gemm_skinny_slices(g.M, g.N, g.Ktot, g.Kpad, slab ? slab_bytes : 0, &tps);
  // the largest tile whose grid still covers the part, else the smallest.  A split layer has fewer than SK_CUS 32 x 32
  // tiles and its slices fit the slab, so its larger tilings never cover the part: it always takes the smallest.
  const long t64 = (long)((g.M + 63) / 64) * ((g.N + 63) / 64);
  const long t32x64 = (long)((g.M + 31) / 32) * ((g.N + 63) / 64);
  if (S == 1 && t64 >= SK_CUS) return run_tile<2, 2>(g, epi, 1, tps, slab, s);
  if (S == 1 && t32x64 >= SK_CUS) return run_tile<1, 2>(g, epi, 1, tps, slab, s);
  INF_TRY((run_tile<1, 1>(g, epi, S, tps, slab, s)));
  if (S == 1) return INF_OK;
  const long rows = (long)((g.M + 31) / 32) * 32;
  const long ne = (long)g.M * g.N;
  const bool prof = prof_enabled();
  if (prof) prof_begin_launch(s);
  hipLaunchKernelGGL(gemm_skinny_reduce_kernel, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, s, g, epi, S, rows,
                     (const float*)slab);
  INF_CHECK_LAUNCH();
  if (prof) {
    const bool dio = epi == EP_MUL_DERIV || (epi >= EP_ACT_SWISH && g.deriv_out);
    prof_end_launch(s, 961, (double)S * ne, 4.0 * ne * (S + 1.0 + (dio ? 1.0 : 0.0)));
  }
  return INF_OK;
}

}  // namespace inf
