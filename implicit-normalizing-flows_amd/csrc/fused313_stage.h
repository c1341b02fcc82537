// Halo staging of the fused 3-1-3 kernels (fused313.hip, fused313k.hip, fused313p.hip): the one copy of the code that
// fills the input halo tile, the im2col offset table with its K-padding zero run, and the per-tile phase-A scale, plus
// the small operand helpers the chunked kernels share.  Everything is __forceinline__ and takes the tile geometry as a
// plain struct of ints, so a kernel instantiated for a compile-time (C, W) still folds the index arithmetic.
#pragma once
#include <type_traits>

#include "kernels.h"

namespace inf {

// pixels of one image row that a bn-pixel tile covers: whole rows of a narrow image, a bn-wide segment of a wide one
constexpr int tile_seg(int W, int bn) { return W < bn ? W : bn; }

// host: an H x W image cuts into bn-pixel tiles of whole rows (W < bn) or of row segments (W >= bn) with no column of
// a tile left over: the only geometry the 128-pixel and the two-per-CU kernels (fused313k.hip, fused313p.hip) take
inline bool halo_tiles_exact(int H, int W, int bn) {
  const int seg = tile_seg(W, bn);
  return (H * W) % bn == 0 && bn % seg == 0 && !(W > bn && W % bn != 0);
}
// host: image rows of one tile.  Whole-row tiles (W <= bn) take as many rows as fit, floor(bn / W), and no more than the
// image has; on an exact shape this is bn / seg
inline int tile_rows(int H, int W, int bn) {
  const int r = bn / tile_seg(W, bn);
  return (W <= bn && H < r) ? H : r;
}
// host: fused313.hip's tiles.  Exact ones, or ragged whole-row tiles: rows * W <= bn live pixel columns and bn - rows * W
// dead ones per tile, the last tile of an image possibly short of rows.  Segment tiles stay exact.
inline bool halo_tiles(int H, int W, int bn) { return W <= bn || W % bn == 0; }
// host: tiles per image (P / bn on an exact shape)
inline int tile_count(int H, int W, int bn) {
  if (W > bn) return H * (W / bn);
  const int rows = tile_rows(H, W, bn);
  return (H + rows - 1) / rows;
}
// host: LDS floats of the im2col offset table, the halo tile and its zero run (what HaloGeom::vhz() + K1pad come to)
inline long halo_lds_floats(int C, int H, int W, int bn) {
  const int seg = tile_seg(W, bn), rows = tile_rows(H, W, bn);
  return (9L * C + 15) / 16 * 16 + (long)C * (rows + 2) * (seg + 2) + (long)rows * (seg + 2);
}

// One tile's geometry: `rows` image rows of `seg` pixels of image `img`, first pixel (y0, x0).  The halo tile is
// [C][rows + 2][seg + 2] floats, followed by a zero run that the K-padding rows of phase A's im2col point at.
struct HaloGeom {
  int C, H, W, seg, rows, K1pad;
  int img, tile, y0, x0;
  __device__ __forceinline__ int P() const { return H * W; }
  __device__ __forceinline__ int RH() const { return rows + 2; }
  __device__ __forceinline__ int CW() const { return seg + 2; }
  __device__ __forceinline__ int vhn() const { return C * RH() * CW(); }
  // phase A reads vh[koff + pix], so the zero run must cover every pixel offset of the tile: rows * CW floats (a
  // single zero slot there once let padded rows read LDS the kernel never wrote)
  __device__ __forceinline__ int vhz() const { return vhn() + rows * CW(); }
  // Ragged whole-row tiles: the rows of this tile that lie in the image (the last tile of an image may be short), and
  // its live pixel columns n < live_cols() (n = row * seg + x); the other columns of the bn are dead.  On an exact
  // shape every column is live.
  __device__ __forceinline__ int live_rows() const { return min(rows, H - y0); }
  __device__ __forceinline__ int live_cols() const { return live_rows() * seg; }
};

// Stages the halo tile into vh[0, vhz) with NT threads; hmx / dacc receive this thread's max |value| and its part of
// the trace partial.  Two inputs:
//  - series chaining (a.in_taps): the input is the previous VJP's packed taps; the tap sum, the preact swish'
//    multiplier, that term's trace partial and the Neumann accumulation (conv_out's OM_VJP work) happen here.  Up to 4
//    halo elements per thread and pass with clamped-address loads, all issued before any is used (44 loads in flight
//    instead of one bounds-checked chain per element); the pass width is wave-uniform and a compile-time constant per
//    branch, so a small halo costs one pass of 11 loads.  after_loads(last) runs between a pass's loads and their use
//    (last: nothing is staged after this pass), for loads a kernel wants queued behind the staging's.
//  - the plain input (forward applies the preact swish): FU elements per thread and pass, again every load from a
//    clamped address issued before any is used.  The values staged do not depend on FU.
// SIDE_ALWAYS: the side inputs (vmul_x, dot_eps, acc_w) are loaded whether the net has them or not (from a dummy
// address where it does not), the form the 64-pixel kernels were measured with; false loads them only where present.
// SIN: the leading activation / the series-chaining derivative may be Sin (every instantiation but the Swish forward
// ones, which only Swish nets launch; the VJP instantiations are shared by all kinds).
template <int NT, int FU, bool SIDE_ALWAYS, bool SIN, class AfterLoads>
__device__ __forceinline__ void stage_halo(const Net313Args& a, const HaloGeom& g, int tid, float* vh, float& hmx,
                                           double& dacc, AfterLoads&& after_loads) {
  const int C = g.C, H = g.H, W = g.W, P = g.P(), seg = g.seg, rows = g.rows, y0 = g.y0, x0 = g.x0;
  const int RH = g.RH(), CW = g.CW(), vhn = g.vhn(), vhz = g.vhz();
  const float* in = a.in ? a.in + (long)g.img * C * P : nullptr;
  if (a.in_taps) {
    const float* ytap = a.in_taps + (long)g.img * (9 * C) * P;
    const float* mx = a.vmul_x ? a.vmul_x + (long)g.img * C * P : nullptr;
    const float* ep = a.dot_eps ? a.dot_eps + (long)g.img * C * P : nullptr;
    const float msp = (a.vmul_x && !a.vmul_act) ? softplus_f(ldc(a.vmul_beta)) : 0.f;
    const float* mxp = mx ? mx : ytap;
    const float* epp = ep ? ep : ytap;
    float* accw = a.acc_w ? a.acc_w + (long)g.img * C * P : nullptr;   // Neumann-vector accumulator
    const float* awp = accw ? accw : ytap;
    auto pass = [&](auto nuc, int i0) {
      constexpr int NU = decltype(nuc)::value;
      float tv[NU][9], xm[NU], ev[NU], wv[NU];
#pragma unroll
      for (int u = 0; u < NU; ++u) {
        const int i = i0 + u * NT;
        const int ic = i < vhn ? i : 0;
        const int c = ic / (RH * CW), rr = ic - c * RH * CW;
        const int hy = rr / CW, hx = rr - hy * CW;
        const int yq = min(max(y0 + hy - 1, 0), H - 1), xq = min(max(x0 + hx - 1, 0), W - 1);
        const long ee = (long)c * P + yq * W + xq;
        const float* yc = ytap + (long)c * 9 * P;
#pragma unroll
        for (int tp = 0; tp < 9; ++tp) {
          const int y2 = min(max(yq + tp / 3 - 1, 0), H - 1), x2 = min(max(xq + tp % 3 - 1, 0), W - 1);
          tv[u][tp] = yc[(long)tp * P + y2 * W + x2];
        }
        // (!SIDE_ALWAYS: side inputs only where the net has them, a dummy load still costs a slot in the wave's load
        // queue)
        xm[u] = (SIDE_ALWAYS || mx) ? mxp[ee] : 0.f;
        ev[u] = (SIDE_ALWAYS || ep) ? epp[ee] : 0.f;
        wv[u] = (SIDE_ALWAYS || accw) ? awp[ee] : 0.f;
      }
      after_loads(i0 - tid + NT * NU >= vhz);
#pragma unroll
      for (int u = 0; u < NU; ++u) {
        const int i = i0 + u * NT;
        const int ic = i < vhn ? i : 0;
        const int c = ic / (RH * CW), rr = ic - c * RH * CW;
        const int hy = rr / CW, hx = rr - hy * CW;
        const int yy = y0 + hy - 1, xx = x0 + hx - 1;
        const bool in_img = i < vhn && yy >= 0 && yy < H && xx >= 0 && xx < W;
        // ok == 2: the tile's own pixels.  A short last tile needs no live_rows() here: its missing rows lie below the
        // image, so in_img already excludes them
        const int ok = in_img ? ((hy >= 1 && hy <= rows && hx >= 1 && hx <= seg) ? 2 : 1) : 0;
        float v = 0.f;
#pragma unroll
        for (int tp = 0; tp < 9; ++tp) {
          const int y2 = yy + tp / 3 - 1, x2 = xx + tp % 3 - 1;
          const bool vt = y2 >= 0 && y2 < H && x2 >= 0 && x2 < W;
          v += vt ? tv[u][tp] : 0.f;
        }
        if (mx) v = v * (a.vmul_act ? fused_act_d<SIN>(a.vmul_act, xm[u]) : swish_fast_d(xm[u], msp));
        v = ok ? v : 0.f;
        if (ep && ok == 2) dacc += (double)v * (double)ev[u];
        if (accw && ok == 2) accw[(long)c * P + yy * W + xx] = fmaf(a.acc_coef, v, wv[u]);
        hmx = fmaxf(hmx, fabsf(v));
        if (i < vhz) vh[i] = v;
      }
    };
    constexpr int SU = 4;
    for (int i0 = tid; i0 < vhz; i0 += NT * SU) {
      const int nu = min(SU, (vhz - (i0 - tid) + NT - 1) / NT);     // wave-uniform
      if (nu >= 4) pass(std::integral_constant<int, 4>(), i0);
      else if (nu == 3) pass(std::integral_constant<int, 3>(), i0);
      else if (nu == 2) pass(std::integral_constant<int, 2>(), i0);
      else pass(std::integral_constant<int, 1>(), i0);
    }
  } else {
    const float pre_sp = a.pre_beta ? softplus_f(ldc(a.pre_beta)) : 0.f;
    for (int i0 = tid; i0 < vhz; i0 += NT * FU) {
      float lv[FU];
      bool ok[FU];
#pragma unroll
      for (int u = 0; u < FU; ++u) {
        const int i = i0 + u * NT;
        const int ic = i < vhn ? i : 0;
        const int c = ic / (RH * CW), rr = ic - c * RH * CW;
        const int hy = rr / CW, hx = rr - hy * CW;
        const int yy = y0 + hy - 1, xx = x0 + hx - 1;
        ok[u] = i < vhn && yy >= 0 && yy < H && xx >= 0 && xx < W;
        lv[u] = in[(long)c * P + min(max(yy, 0), H - 1) * W + min(max(xx, 0), W - 1)];
      }
#pragma unroll
      for (int u = 0; u < FU; ++u) {
        const int i = i0 + u * NT;
        float v = 0.f;
        if (ok[u]) {
          v = lv[u];
          if (a.pre_beta) v = swish_fast_f(v, pre_sp);
          else if (a.pre_act) v = fused_act_f<SIN>(a.pre_act, v);
        }
        hmx = fmaxf(hmx, fabsf(v));
        if (i < vhz) vh[i] = v;
      }
    }
  }
}

// this wave's halo maximum / trace partial into its LDS slot (read after the staging barrier)
__device__ __forceinline__ void put_wave_max(int lane, int wid, float hmx, float* hmax) {
  const float w = wave_max(hmx);
  if (lane == 0) hmax[wid] = w;
}
__device__ __forceinline__ void put_wave_dot(const Net313Args& a, int lane, int wid, double dacc, double* red) {
  if (a.dot_part) {
    const double w = wave_sum(dacc);
    if (lane == 0) red[wid] = w;
  }
}

// after the staging barrier: the tile's trace partial, the NW wave sums in wave order
template <int NW>
__device__ __forceinline__ void write_dot_part(const Net313Args& a, const HaloGeom& g, int tid, const double* red) {
  if (a.dot_part && tid == 0) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < NW; ++w) s += red[w];
    a.dot_part[(long)g.img * a.dot_nchunk + g.tile] = s;
  }
}

// im2col table: halo offset of K row k = (channel, tap); the K-padding rows point at the zero run
template <int NT>
__device__ __forceinline__ void fill_koff(const HaloGeom& g, int tid, int* koff) {
  for (int k = tid; k < g.K1pad; k += NT) {
    int o = g.vhn();
    if (k < 9 * g.C) {
      const int c = k / 9, tt = k - c * 9;
      o = c * g.RH() * g.CW() + (tt / 3) * g.CW() + (tt % 3);
    }
    koff[k] = o;
  }
}

// phase A's scale (INF_MFMA_F16X3): one per tile, from the halo maximum over all NW waves; eA unscales its results
template <int NW>
__device__ __forceinline__ void phaseA_scale(const Net313Args& a, const float* hmax, float& sA, int& eA) {
  float m_ = 0.f;
#pragma unroll
  for (int w = 0; w < NW; ++w) m_ = fmaxf(m_, hmax[w]);
  const int sc = h3_scale_exp(m_);
  sA = __builtin_amdgcn_ldexpf(1.f, sc);
  eA = -(sc + ldc(a.Ah_exp));
}

// the two (h, l) planes of fragment tile `tile` (fragment-major, launch_split2h order)
__device__ __forceinline__ void ldw2(const u32x4* base, long tile, int lane, u32x4 (&o)[2]) {
  const u32x4* q = base + tile * 2 * 64 + lane;
  o[0] = q[0];
  o[1] = q[64];
}

// 4 consecutive fp32 values (rows q = 0..3 of one accumulator group) -> scaled fp16 h / l pieces, packed
__device__ __forceinline__ void split4h(float v0, float v1, float v2, float v3, float S, uint2& h, uint2& l) {
  const _Float16 h0 = (_Float16)(v0 * S), h1 = (_Float16)(v1 * S), h2 = (_Float16)(v2 * S), h3 = (_Float16)(v3 * S);
  const _Float16 l0 = (_Float16)__builtin_fmaf(v0, S, -(float)h0), l1 = (_Float16)__builtin_fmaf(v1, S, -(float)h1);
  const _Float16 l2 = (_Float16)__builtin_fmaf(v2, S, -(float)h2), l3 = (_Float16)__builtin_fmaf(v3, S, -(float)h3);
  const f16x2 a = {h0, h1}, b = {h2, h3}, c = {l0, l1}, d = {l2, l3};
  h = make_uint2(__builtin_bit_cast(unsigned, a), __builtin_bit_cast(unsigned, b));
  l = make_uint2(__builtin_bit_cast(unsigned, c), __builtin_bit_cast(unsigned, d));
}

}  // namespace inf
