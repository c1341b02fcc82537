// One launch per imBlock evaluation of a fused fc block (tabular / toy nets: d <= 8 features, 128-wide hidden layers,
// f16x3 arithmetic): implicit_block.py:220-260,358-362 with broyden.py:123-193 in between, device-resident.
//
// A workgroup owns BK_S = 48 samples for the whole block and keeps their Broyden state in LDS:
//   phase 1  log|det(I + J_fx(x))| and x_embed = f_x(x) + x (forward-mode tangents, 3 passes of 16 samples x (d + 1)
//            columns, fcnet_h3.hip's JAC arithmetic and LU),
//   phase 2  the root solve of g(z) = x_embed - f_z(z) - z from z = 0: per iteration the low-rank update (U / VT columns
//            in LDS), the net f_z on the 48 columns with its weights held in registers across iterations, the residual
//            and its per-sample sum of squares.  The global rule (broyden.py:131,153-172: one Frobenius norm over the
//            batch) exchanges one fp64 partial per workgroup per iteration through tagged granules (every workgroup
//            sums them in the same order, so every workgroup takes the same decision); the per-sample rule
//            (INF_CONV_PER_SAMPLE) needs no exchange.  The lowest iterate and its f are kept per sample.
//   phase 3  z = (f_x(x) - f_z(z*)) + x (implicit_block.py:74-80,227) and log|det(I + J_fz(z))|.
// The host reads the block's statistics once.  A protective break (broyden.py:169-172) is reported, not handled: the host
// then runs the Banach fallback (engine.hip banach_solve) on the buffers phase 1 / 2 leave in global memory.
//
// The global rule needs every workgroup resident at once: the host launches it cooperatively (the launch fails rather
// than deadlocks when the grid does not fit), and every spin is bounded (a timeout sets the error word and the workgroup
// leaves; the host reports INF_ERR_HIP).
#include <cstdio>
#include <cstring>
#include <utility>

#include "fcblock_pass.h"

namespace inf {

namespace {
constexpr unsigned BK_SPIN_MAX = 1u << 22;
constexpr int BK_NSETS = 4;       // granule sets of the global rule's exchange (gather_k)

typedef __attribute__((address_space(1))) unsigned long long gu64;
typedef __attribute__((address_space(1))) unsigned int gu32;

// ---- the global rule's exchange: one fp64 per workgroup and iteration as two tagged 32-bit granules -------------------
// (the R2 form of cdna_hip_programming.md Guideline 16: the data is the flag; 8-byte relaxed agent-scope stores and
// loads, no fence).  Two granule sets alternate between iterations: a workgroup can only write set (k & 1) again at
// iteration k + 2, after every workgroup has written iteration k + 1, i.e. after every workgroup has read iteration k.
__device__ __forceinline__ void publish(gu64* g, unsigned tag, double v) {
  const unsigned long long bits = (unsigned long long)__double_as_longlong(v);
  __hip_atomic_store(g + 0, ((unsigned long long)tag << 32) | (bits >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(g + 1, ((unsigned long long)tag << 32) | (bits & 0xffffffffull), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}
// wave 0: the sum over workgroups (in workgroup order per lane, then a fixed butterfly: the same bits in every
// workgroup).  The granules are read 512 at a time (8 per lane), in order, so any grid size is covered.  Returns false
// on timeout.
__device__ __forceinline__ bool gather_total(const gu64* g, unsigned tag, int nwg, int lane, double& total) {
  const int n = 2 * nwg;        // granules; lane holds indices base + lane + 64 q
  double s = 0.0;
  for (int base = 0; base < n; base += 512) {
    unsigned long long v[8];
    for (unsigned spins = 0;; ++spins) {
      bool ok = true;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int i = base + lane + 64 * q;
        if (i < n) {
          v[q] = __hip_atomic_load(g + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          ok &= (unsigned)(v[q] >> 32) == tag;
        } else {
          v[q] = 0;
        }
      }
      if (__all(ok)) break;
      if (spins > BK_SPIN_MAX) return false;
      __builtin_amdgcn_s_sleep(2);
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const unsigned lo = (unsigned)__shfl_down((int)(unsigned)v[q], 1, 64);   // the odd granule of the pair
      const int i = base + lane + 64 * q;
      if (!(lane & 1) && i < n) {
        const unsigned long long bits = ((v[q] & 0xffffffffull) << 32) | lo;
        s += __longlong_as_double((long long)bits);
      }
    }
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) s += __shfl_xor(s, o, 64);
  total = s;
  return true;
}

// The Broyden update of one sample (broyden.py:174-181 with update = -matvec(...), then x_new = x + update; the algebra
// and accumulation order of fcnet_common.h broyden_update_fc), state in LDS: U / VT columns [j][s][i], vectors [s][i].
template <int DD>
__device__ __forceinline__ void bk_update(float* U, float* VT, int S, int s, int m, int ncols, const float* x,
                                          const float* gx_, const float* dx_, const float* dg_, float* xnew,
                                          float* dxnew) {
  const int o = s * DD;
  float dx[DD], dg[DD], vt[DD], t[DD];
#pragma unroll
  for (int i = 0; i < DD; ++i) {
    dx[i] = dx_[o + i];
    dg[i] = dg_[o + i];
    vt[i] = -dx[i];
    t[i] = -dg[i];
  }
  for (int j = 0; j < m; ++j) {
    const float* Uj = U + ((long)j * S + s) * DD;
    const float* Vj = VT + ((long)j * S + s) * DD;
    float u[DD], v[DD];
#pragma unroll
    for (int i = 0; i < DD; ++i) {
      u[i] = Uj[i];
      v[i] = Vj[i];
    }
    double sa = 0.0, sc = 0.0;
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
  float um[DD];
  double den = 0.0;
#pragma unroll
  for (int i = 0; i < DD; ++i) {
    um[i] = dx[i] - t[i];
    den += (double)vt[i] * dg[i];
  }
  const float denf = (float)den;
  float* Um = U + ((long)m * S + s) * DD;
  float* Vm = VT + ((long)m * S + s) * DD;
#pragma unroll
  for (int i = 0; i < DD; ++i) {
    float u = um[i] / denf;
    if (vt[i] != vt[i]) vt[i] = 0.f;
    if (u != u) u = 0.f;
    um[i] = u;
    Vm[i] = vt[i];
    Um[i] = u;
  }
  float gx[DD], tt[DD];
#pragma unroll
  for (int i = 0; i < DD; ++i) {
    gx[i] = gx_[o + i];
    tt[i] = -gx[i];
  }
  for (int j = 0; j < ncols; ++j) {
    float u[DD], v[DD];
    if (j == m) {
#pragma unroll
      for (int i = 0; i < DD; ++i) {
        u[i] = um[i];
        v[i] = vt[i];
      }
    } else {
      const float* Uj = U + ((long)j * S + s) * DD;
      const float* Vj = VT + ((long)j * S + s) * DD;
#pragma unroll
      for (int i = 0; i < DD; ++i) {
        u[i] = Uj[i];
        v[i] = Vj[i];
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
    const float x0 = x[o + i];
    const float xe = x0 + (-tt[i]);
    xnew[o + i] = xe;
    dxnew[o + i] = xe - x0;
  }
}

// LDS carve (dynamic shared memory; every offset a multiple of 16)
struct BkLayout {
  int S, DD, T;
  size_t vec, ps_d, ps_i, ring, ctl, uni, jac, fwd_uv, fwd, wts, total;
};
__host__ __device__ inline BkLayout bk_layout(int DD, int T) {
  BkLayout L;
  L.S = BK_S;
  L.DD = DD;
  L.T = T;
  size_t off = 0;
  L.vec = off;                                  // V_COUNT per-sample vectors [s][i] fp32
  off += bk_al(sizeof(float) * 12 * BK_S * DD);
  L.ps_d = off;                                 // per-sample doubles: init, lowest
  off += bk_al(sizeof(double) * 2 * BK_S);
  L.ps_i = off;                                 // per-sample ints: nstep, lowest_step, prot, active, improved
  off += bk_al(sizeof(int) * 5 * BK_S);
  L.ring = off;                                 // per-sample objective ring [s][T] (per-sample rule's stall test)
  off += bk_al(sizeof(double) * BK_S * T);
  L.ctl = off;                                  // decisions, partial sums
  off += bk_al(sizeof(double) * 80);
  L.uni = off;                                  // union: JAC scratch | U, VT + FWD scratch
  const int jnc = 16 * (DD + 1);
  const size_t jac = bk_al(2 * sizeof(uint16_t) * jnc * FC_LD) + bk_al(sizeof(float) * 16 * jnc) +
                     bk_al(sizeof(float) * FC_NW * jnc) + bk_al(sizeof(int) * jnc);
  L.jac = L.uni;
  L.fwd_uv = L.uni;
  const size_t uv = bk_al(sizeof(float) * 2 * (size_t)T * BK_S * DD);
  L.fwd = L.uni + uv;
  const size_t fwd = bk_al(2 * sizeof(uint16_t) * BK_S * FC_LD) + bk_al(sizeof(float) * 16 * BK_S) +
                     bk_al(sizeof(float) * FC_NW * BK_S) + bk_al(sizeof(int) * BK_S);
  L.wts = L.uni + bk_al(jac > uv + fwd ? jac : uv + fwd);   // the solved net's input / output layer planes
  L.total = L.wts + sizeof(u32x4) * (BK_W0_VEC + BK_WO_VEC);
  return L;
}

enum { V_XEMB = 0, V_FX, V_XIN, V_X, V_G, V_DX, V_DG, V_XLOW, V_FLOW, V_FCUR, V_XP, V_FP, V_COUNT };
enum { I_NSTEP = 0, I_LSTEP, I_PROT, I_ACT, I_IMP };
enum { C_GO = 0, C_STOP, C_IMP, C_ERR, C_ANY, C_PROT };
}  // namespace

// forward-mode Jacobian of one net over the workgroup's samples (three passes of 16 samples): per sample, f(in) + bias
// into f_out (and f + in into emb_out, when given) and log|det(I + J)| into logdet[b] (b < B)
template <int DD, int ACT, int NH>
__device__ __forceinline__ void bk_jacobian(const FcArgs& a, char* jbase, const float* in, float* f_out, float* emb_out,
                                            float* logdet, long b0, int B, Stamps* ts) {
  constexpr int NCB = DD + 1;
  constexpr int NC = 16 * NCB;
  const Pass P = bk_pass(jbase, NC);
  const int tid = threadIdx.x;
  const float* bias = a.L[NH + 1].b;
  bk_sync();                                   // the caller's per-sample inputs
  for (int q = 0; q < BK_FCB; ++q) {
    for (int i = tid; i < 16 * NC; i += FC_NT) {
      const int k = i / NC, c = i - k * NC;
      const int cb = c >> 4, sl = c & 15;
      const int s = 16 * q + sl;
      float v = 0.f;
      if (k < DD && b0 + s < B) v = cb > 0 ? (k == cb - 1 ? 1.f : 0.f) : in[s * DD + k];
      P.tmp[i] = v;
    }
    mlp_jac2<DD, NCB, ACT, NH>(a, P, ts);
    if (tid < 16) {
      const int s = 16 * q + tid;
      const long b = b0 + s;
      if (b < B) {
#pragma unroll
        for (int i = 0; i < DD; ++i) {
          const float v = P.tmp[i * NC + tid] + bias[i];
          f_out[s * DD + i] = v;
          if (emb_out) emb_out[s * DD + i] = v + in[s * DD + i];
        }
        logdet[b] = logdet_lu<DD>([&](int i, int j) { return P.tmp[i * NC + (j + 1) * 16 + tid]; });
      }
    }
    bk_sync();
    BK_STAMP(ts);
  }
}

template <int DD, int ACT, int NH>
__global__ __launch_bounds__(FC_NT) void fcblock_kernel(FcBlockArgs a) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const BkLayout Ly = bk_layout(DD, a.T);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int B = a.B, T = a.T, wg = blockIdx.x, nwg = gridDim.x;
  const long b0 = (long)wg * BK_S;
  constexpr int S = BK_S;
  constexpr int NC = BK_S;
  const bool per_sample = a.per_sample != 0;
  float* vec = reinterpret_cast<float*>(lds + Ly.vec);
  auto V = [&](int k) { return vec + (size_t)k * S * DD; };
  double* psd = reinterpret_cast<double*>(lds + Ly.ps_d);   // [0, S) init, [S, 2S) lowest
  int* psi = reinterpret_cast<int*>(lds + Ly.ps_i);
  auto PI = [&](int k) { return psi + k * S; };
  double* ring = reinterpret_cast<double*>(lds + Ly.ring);
  double* cd = reinterpret_cast<double*>(lds + Ly.ctl);      // [0] total, [1] init, [2] lowest, [8, 72) trace
  int* ctl = reinterpret_cast<int*>(cd + 72);
  char* ubase = lds + Ly.uni;
  const bool mine = tid < S;                                  // the sample thread of the update / FWD epilogue
  const bool valid_t = mine && b0 + tid < B;
  Stamps tsv{a.tbuf, 0};
  Stamps* ts = &tsv;
  BK_STAMP(ts);

  // ---- phase 1 (jp = 0): x in the per-sample layout, log|det(I + J_fx(x))|, f_x(x), x_embed;
  // ---- phase 3 (jp = 1, after the solve): z = (f_x(x) - f_z(z*)) + x, log|det(I + J_fz(z))|
  // (one instance of the Jacobian pass, and one of the solve's net pass below: the kernel's code stays in the
  // instruction cache)
  for (int jp = 0; jp < 2; ++jp) {
  if (jp == 0) {
    for (int i = tid; i < S * DD; i += FC_NT) {
      const int s = i / DD, k = i - s * DD;
      const long b = b0 + s;
      float v = 0.f;
      if (b < B) {
        v = a.x[b * DD + k];
        a.xin_g[(long)k * B + b] = v;
      }
      V(V_XIN)[i] = v;
    }
  } else {
    for (int i = tid; i < S * DD; i += FC_NT) {
      const int s = i / DD;
      const long b = b0 + s;
      const float v = (V(V_FX)[i] - V(V_FLOW)[i]) + V(V_XIN)[i];
      V(V_X)[i] = v;
      if (b < B) a.z[b * DD + (i - s * DD)] = v;
    }
  }
  bk_jacobian<DD, ACT, NH>(jp ? a.nz : a.nx, ubase, jp ? V(V_X) : V(V_XIN), jp ? V(V_G) : V(V_FX),
                           jp ? nullptr : V(V_XEMB), jp ? a.logdet_z : a.logdet_x, b0, B, ts);
  if (jp == 1) break;
  if (valid_t) {
#pragma unroll
    for (int i = 0; i < DD; ++i) {
      a.fx_g[(long)i * B + b0 + tid] = V(V_FX)[tid * DD + i];
      a.xemb_g[(long)i * B + b0 + tid] = V(V_XEMB)[tid * DD + i];
    }
  }

  // ---- phase 2: the root solve from z = 0
  NetRegs<NH> R;
  load_net<NH>(a.nz, w, lane, reinterpret_cast<u32x4*>(lds + Ly.wts), R);
  float* U = reinterpret_cast<float*>(ubase);
  float* VT = U + (size_t)T * S * DD;
  const Pass P = bk_pass(lds + Ly.fwd, S);
  const float* bias_z = a.nz.L[NH + 1].b;
  const double eps = a.eps, eps_ps = a.eps_ps;
  // f_z at the iterate in tmp rows [0, DD) (V_X holds the same values); per sample thread: f -> fcur, g -> g, the
  // sum of squares of g returned (0 elsewhere)
  auto residual = [&]() -> double {
    mlp_pass<DD, BK_FCB, false, ACT, NH, true>(a.nz, &R, P, ts);
    double acc = 0.0;
    if (valid_t) {
#pragma unroll
      for (int i = 0; i < DD; ++i) {
        const float f = P.tmp[i * NC + tid] + bias_z[i];
        const float gx = (V(V_XEMB)[tid * DD + i] - f) - V(V_X)[tid * DD + i];
        V(V_FCUR)[tid * DD + i] = f;
        V(V_G)[tid * DD + i] = gx;
        acc += (double)gx * (double)gx;
      }
    }
    return acc;
  };
  // global rule, the exchange of step k's sum of squares: wave 0 publishes the workgroup's partial (two granules in set
  // k % BK_NSETS), then one agent-scope counter add per workgroup; gather_k waits for the counter, reads every
  // workgroup's granules (tag-checked) and sums them in workgroup order and a fixed butterfly (the same bits in every
  // workgroup) into cd[0].  Between publishing step k and gathering it, the workgroup computes step k + 1 (speculative,
  // discarded when step k stops the solve), so the exchange's latency and the workgroups' skew are hidden.  A workgroup
  // publishes step k only after it gathered step k - 2, so the oldest set still being read is k - 3's: four sets.
  gu64* gran = (gu64*)a.gran;
  gu32* cnt = ((gu32*)a.error) + 1;
  auto publish_k = [&](double part, int k) {
    if (w == 0) {
      double sp = part;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) sp += __shfl_xor(sp, o, 64);
      if (lane == 0) {
        publish(gran + ((size_t)(k % BK_NSETS) * nwg + wg) * 2, a.tag0 + (unsigned)k, sp);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  };
  auto gather_k = [&](int k) -> bool {
    if (w == 0) {
      int ok = 1;
      if (lane == 0) {
        const unsigned target = (unsigned)nwg * (unsigned)(k + 1);
        for (unsigned spins = 0; __hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target; ++spins) {
          if (spins > BK_SPIN_MAX) {
            ok = 0;
            break;
          }
          __builtin_amdgcn_s_sleep(1);
        }
      }
      ok = __shfl(ok, 0, 64);
      double t = 0.0;
      if (ok) ok = gather_total(gran + (size_t)(k % BK_NSETS) * nwg * 2, a.tag0 + (unsigned)k, nwg, lane, t);
      if (lane == 0) {
        cd[0] = t;
        ctl[C_ERR] = ok ? 0 : 1;
      }
    }
    bk_sync();
    BK_STAMP(ts);
    return ctl[C_ERR] == 0;
  };
  // thread 0: the decision of step j (broyden.py:145-172) from cd[0]; ctl[C_IMP] / ctl[C_STOP]
  auto decide = [&](int j) {
    const double obj = sqrt(cd[0]);
    int imp = 0, stop = 0;
    if (j == 0) {                                                  // :144-153
      cd[1] = cd[2] = obj;                                         // init, lowest
      cd[8] = obj;                                                 // trace[0]
      ctl[C_ANY] = 0;                                              // lowest_step
      ctl[C_PROT] = 0;
      stop = (obj >= eps && T > 0) ? 0 : 1;
    } else {
      const int nt = j + 1;                                        // trace entries (<= T + 1 <= 31)
      cd[8 + j] = obj;
      if (obj < cd[2]) {                                           // :159-162
        cd[2] = obj;
        ctl[C_ANY] = j;
        imp = 1;
      }
      if (obj < eps) {                                             // :163
        stop = 1;
      } else {
        if (obj < 3 * eps && j == T) {                             // :165-168 (trace[-T:])
          const int k0 = nt > T ? nt - T : 0;
          double mx = cd[8 + k0], mn = mx;
          for (int q = k0; q < nt; ++q) {
            mx = fmax(mx, cd[8 + q]);
            mn = fmin(mn, cd[8 + q]);
          }
          if (mx / mn < 1.3) stop = 1;
        }
        if (!stop && obj > cd[1] * 1e6) {                          // :169-172
          ctl[C_PROT] = 1;
          stop = 1;
        }
        if (j >= T) stop = 1;                                      // :153
      }
    }
    ctl[C_IMP] = imp;
    ctl[C_STOP] = stop;
  };
  if (mine) {
#pragma unroll
    for (int i = 0; i < DD; ++i) V(V_X)[tid * DD + i] = 0.f;                  // x0 = 0
  }
  bool fin = false, err = false;
  int k = -1, nstep = 0;
  while (!fin) {
    k += 1;
    // x_k: step 1 is x0 + (-g0); later steps the low-rank update from step k - 1 (column (k - 2) % T); into the net's
    // input rows and V_X, dx_k into V_DX; g_{k-1} kept for dg
    const bool act = valid_t && (k == 0 || !per_sample || PI(I_ACT)[tid]);
    float gprev[DD];
    if (mine) {
#pragma unroll
      for (int i = 0; i < DD; ++i) gprev[i] = k ? V(V_G)[tid * DD + i] : 0.f;
      if (act && k > 0) {
        if (k == 1) {
#pragma unroll
          for (int i = 0; i < DD; ++i) V(V_FCUR)[tid * DD + i] = V(V_X)[tid * DD + i] + (-gprev[i]);
        } else {
          bk_update<DD>(U, VT, S, tid, (k - 2) % T, min(k - 1, T), V(V_X), V(V_G), V(V_DX), V(V_DG), V(V_FCUR),
                        V(V_DX));
        }
#pragma unroll
        for (int i = 0; i < DD; ++i) {
          const float x0 = V(V_X)[tid * DD + i], xe = V(V_FCUR)[tid * DD + i];
          if (k == 1) V(V_DX)[tid * DD + i] = xe - x0;
          V(V_X)[tid * DD + i] = xe;
        }
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) P.tmp[i * NC + tid] = i < DD ? V(V_X)[tid * DD + i] : 0.f;
    }
    const double pk = residual();
    if (mine) {
#pragma unroll
      for (int i = 0; i < DD; ++i) {
        if (k == 0) {                              // the lowest iterate starts as x0 and f(0) (broyden.py:150)
          V(V_XLOW)[tid * DD + i] = 0.f;
          V(V_FLOW)[tid * DD + i] = V(V_FCUR)[tid * DD + i];
        } else if (act) {
          V(V_DG)[tid * DD + i] = V(V_G)[tid * DD + i] - gprev[i];
        } else {
          V(V_G)[tid * DD + i] = gprev[i];          // a frozen sample keeps its state
        }
      }
    }
    if (!per_sample) {
      publish_k(pk, k);
      // decide step k - 1 (step k was computed meanwhile), and step k itself when it is the threshold's
      int j = k - 1;
      for (;;) {
        if (j >= 0) {
          if (!gather_k(j)) {
            err = fin = true;
            break;
          }
          if (tid == 0) decide(j);
          bk_sync();
          const bool imp = ctl[C_IMP] != 0, stop = ctl[C_STOP] != 0;
          if (imp && mine) {
            const float* xs = j == k ? V(V_X) : V(V_XP);
            const float* fs = j == k ? V(V_FCUR) : V(V_FP);
#pragma unroll
            for (int i = 0; i < DD; ++i) {
              V(V_XLOW)[tid * DD + i] = xs[tid * DD + i];
              V(V_FLOW)[tid * DD + i] = fs[tid * DD + i];
            }
          }
          bk_sync();                             // (ctl is rewritten by the next decision)
          if (stop) {
            nstep = j;
            fin = true;
            break;
          }
        }
        if (j == k) break;
        if (mine) {                              // x_k, f_k for their decision in the next pass
#pragma unroll
          for (int i = 0; i < DD; ++i) {
            V(V_XP)[tid * DD + i] = V(V_X)[tid * DD + i];
            V(V_FP)[tid * DD + i] = V(V_FCUR)[tid * DD + i];
          }
        }
        if (k < T) break;
        j = k;                                   // the threshold: no step beyond it
      }
    } else {
      if (k == 0) {
        if (valid_t) {
          const double obj = sqrt(pk);
          psd[tid] = psd[S + tid] = obj;
          PI(I_NSTEP)[tid] = PI(I_LSTEP)[tid] = PI(I_PROT)[tid] = 0;
          PI(I_ACT)[tid] = (obj >= eps_ps && T > 0) ? 1 : 0;
        } else if (mine) {
          PI(I_ACT)[tid] = 0;
        }
      } else if (act) {
        const double obj = sqrt(pk);
        double* rs = ring + (size_t)tid * T;
        PI(I_NSTEP)[tid] = k;
        rs[(k - 1) % T] = obj;
        if (obj < psd[S + tid]) {                                  // :159-162
          psd[S + tid] = obj;
          PI(I_LSTEP)[tid] = k;
#pragma unroll
          for (int i = 0; i < DD; ++i) {
            V(V_XLOW)[tid * DD + i] = V(V_X)[tid * DD + i];
            V(V_FLOW)[tid * DD + i] = V(V_FCUR)[tid * DD + i];
          }
        }
        int still = 1;
        if (obj < eps_ps) {
          still = 0;
        } else {
          if (obj < 3 * eps_ps && k == T) {
            double mx = rs[0], mn = rs[0];
            for (int j = 1; j < T; ++j) {
              mx = fmax(mx, rs[j]);
              mn = fmin(mn, rs[j]);
            }
            if (mx / mn < 1.3) still = 0;
          }
          if (still && obj > psd[tid] * 1e6) {
            PI(I_PROT)[tid] = 1;
            still = 0;
          }
          if (k >= T) still = 0;
        }
        PI(I_ACT)[tid] = still;
      }
      fin = __syncthreads_or(valid_t && PI(I_ACT)[tid]) == 0;
    }
  }
  const int prot = per_sample ? 0 : ctl[C_PROT];
  bk_sync();

  // statistics, and the buffers the host's Banach fallback (protective break) starts from
  if (!per_sample) {
    if (wg == 0 && tid == 0) {
      FcBlockStats* st = a.stats;
      st->nstep = nstep;
      st->lowest_step = ctl[C_ANY];
      st->prot_break = prot;
      st->n_trace = nstep + 1;
      st->lowest = cd[2];
      for (int j = 0; j <= nstep && j < 64; ++j) st->trace[j] = cd[8 + j];
    }
  } else if (valid_t) {
    const long b = b0 + tid;
    a.s_nstep[b] = PI(I_NSTEP)[tid];
    a.s_lstep[b] = PI(I_LSTEP)[tid];
    a.s_prot[b] = PI(I_PROT)[tid];
    a.s_lowest[b] = psd[S + tid];
  }
  if (err && tid == 0) __hip_atomic_store(((gu32*)a.error), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (valid_t) {
#pragma unroll
    for (int i = 0; i < DD; ++i) {
      a.lowx_g[(long)i * B + b0 + tid] = V(V_XLOW)[tid * DD + i];
      a.lowf_g[(long)i * B + b0 + tid] = V(V_FLOW)[tid * DD + i];
    }
  }
  if (err || prot) return;
  }  // jp
}

size_t fcblock_lds_bytes(int d, int T) { return bk_layout(d, T).total; }

int fcblock_supported(const FcBlockArgs& a) {
  if (a.T <= 0 || a.T > 30 || a.B <= 0) return 0;
  if (a.nx.nl != a.nz.nl || a.nx.d != a.nz.d || a.nx.act != a.nz.act) return 0;
  for (int l = 0; l < a.nx.nl; ++l)
    if (!a.nx.L[l].Ah || !a.nz.L[l].Ah) return 0;
  return fc_block_instance(a.nx.d, a.nx.nl - 2, a.nx.act);
}

int fcblock_grid(int B) { return (B + BK_S - 1) / BK_S; }

int launch_fcblock(const FcBlockArgs& a, hipStream_t s) {
  if (!fcblock_supported(a)) return INF_ERR_UNSUPPORTED;
  const int d = a.nx.d, nh = a.nx.nl - 2;
  const size_t lds = fcblock_lds_bytes(d, a.T);
  const unsigned nb = (unsigned)fcblock_grid(a.B);
  const void* fn = nullptr;
#define BK_PICK(DD_, ACT_, NH_) \
  if (d == DD_ && a.nx.act == ACT_ && nh == NH_) fn = reinterpret_cast<const void*>(&fcblock_kernel<DD_, ACT_, NH_>);
  FC_BLOCK_INSTANCES(BK_PICK)
#undef BK_PICK
  // dynamic LDS beyond the default limit: raised per kernel to what this launch needs (static LDS + dynamic <= 160 KiB)
  static thread_local std::pair<const void*, size_t> attr_set[6] = {};
  bool done = false;
  for (auto& p : attr_set) done = done || (p.first == fn && p.second >= lds);
  if (!done) {
    INF_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    for (auto& p : attr_set)
      if (!p.first || p.first == fn) {
        p = {fn, lds};
        break;
      }
  }
  FcBlockArgs args = a;
  static unsigned long long* tb = nullptr;
  if (INFLOW_PHASE_STAMPS) {
    if (!tb && hipMallocManaged(&tb, sizeof(unsigned long long) * BK_TSLOTS * 1024) != hipSuccess) return INF_ERR_HIP;
    memset(tb, 0, sizeof(unsigned long long) * BK_TSLOTS * 1024);
    args.tbuf = nb <= 1024 ? tb : nullptr;
  }
  void* kargs[] = {&args};
  const bool prof = prof_enabled();
  if (prof) prof_begin_launch(s);
  if (a.per_sample) {
    INF_HIP(hipLaunchKernel(fn, dim3(nb), dim3(FC_NT), kargs, lds, s));
  } else {
    const hipError_t e = hipLaunchCooperativeKernel(fn, dim3(nb), dim3(FC_NT), kargs, (unsigned)lds, s);
    if (e == hipErrorCooperativeLaunchTooLarge) {
      (void)hipGetLastError();
      return INF_ERR_UNSUPPORTED;
    }
    if (e != hipSuccess) {
      set_hip_error(e);
      return INF_ERR_HIP;
    }
  }
  if (INFLOW_PHASE_STAMPS && args.tbuf) {     // per-stage means over the workgroups, in clocks
    INF_HIP(hipStreamSynchronize(s));
    fprintf(stderr, "fcblock stamps (B=%d, %u workgroups): stage mean_clk", a.B, nb);
    for (int i = 1; i < BK_TSLOTS; ++i) {
      double sum = 0.0;
      int n = 0;
      for (unsigned w = 0; w < nb; ++w) {
        const unsigned long long t1 = tb[(long)w * BK_TSLOTS + i], t0 = tb[(long)w * BK_TSLOTS + i - 1];
        if (t1 && t0) {
          sum += (double)(t1 - t0);
          ++n;
        }
      }
      if (!n) break;
      fprintf(stderr, " %d:%.0f", i, sum / n);
    }
    fprintf(stderr, "\n");
  }
  if (prof) {
    // flops: the two Jacobians and f(0) (the solve's later evaluations depend on its step count, which the caller
    // reads from the statistics)
    const double f = fc_flops_per_column(d, a.nx.nl) * a.B * (2.0 * (d + 1) + 1.0);
    prof_end_launch(s, 610, f, 4.0 * a.B * d * 4.0, 3.0 * f / PEAK_BF16_FLOPS_PER_MS);
  }
  return INF_OK;
}

}  // namespace inf

// The series kernel is compiled in this translation unit: on its own the same source gets another register allocation
// (DESIGN.md section 24), and its machine code is held to the parent's.
#include "fcseries.inc"
