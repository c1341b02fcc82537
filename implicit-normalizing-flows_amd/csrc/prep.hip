// Operand preparation, run when a net's weights change (inf_net_refresh): the spectral scale of a layer, the packed
// (and Lipschitz-normalised) GEMM / fused-kernel operands, their exact three-way bf16 split, the scaled two-piece fp16
// split with its scale exponent, and the k-permuted copy of the fp16 planes.  Maps mixed_lipschitz.py:126-132, 320-326,
// 378-386 (sigma = u . W v and the division by max(1, sigma / coeff)); the splits are common.h's split3 / split2h.
#include <algorithm>

#include "kernels.h"

namespace inf {

// sigma partials: one thread per output element (o, y, x) and input-channel chunk (blockIdx.y):
// sum_c (W v)[o,y,x] * u[o,y,x].  Splitting the channel sum over the grid keeps the small-cout layers
// (the 512 -> C output conv: cout*H*W = 3072 elements, 4608 MACs each) from running as 12 serial blocks.
__global__ __launch_bounds__(256) void sigma_partial_kernel(const float* W, const float* u, const float* v, int cout,
                                                            int cin, int ks, int H, int Wd, int cchunk, double* part) {
  __shared__ double red[16];
  const int P = H * Wd;
  const long n = (long)cout * P;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int c0 = blockIdx.y * cchunk, c1 = min(cin, c0 + cchunk);
  double val = 0.0;
  if (i < n) {
    const int o = i / P, p = i - (long)o * P;
    const int y = p / Wd, x = p - y * Wd;
    const int pad = ks / 2;
    float s = 0.f;
    for (int c = c0; c < c1; ++c)
      for (int dy = 0; dy < ks; ++dy)
        for (int dx = 0; dx < ks; ++dx) {
          const int yy = y + dy - pad, xx = x + dx - pad;
          if (yy >= 0 && yy < H && xx >= 0 && xx < Wd)
            s += W[(((long)o * cin + c) * ks + dy) * ks + dx] * v[((long)c * H + yy) * Wd + xx];
        }
    val = (double)s * (double)u[i];
  }
  val = block_sum(val, red);
  if (threadIdx.x == 0) part[(long)blockIdx.y * gridDim.x + blockIdx.x] = val;
}
__global__ __launch_bounds__(256) void sigma_final_kernel(const double* part, int nparts, float coeff, float* factor) {
  __shared__ double red[16];
  double s = 0.0;
  for (int i = threadIdx.x; i < nparts; i += blockDim.x) s += part[i];
  s = block_sum(s, red);
  if (threadIdx.x != 0) return;
  const float sigma = (float)s;
  const float r = sigma / coeff;
  factor[0] = r > 1.f ? r : 1.f;    // torch.max(ones(1), sigma / coeff)
  factor[1] = sigma;
}
int launch_sigma(const float* W, const float* u, const float* v, int cout, int cin, int ks, int H, int Wd,
                 float coeff, float* factor_out, float* scratch, hipStream_t s) {
  const long n = (long)cout * H * Wd;
  const int nb = (int)((n + 255) / 256);
  // channel chunks so that ~2048 blocks run; never more than SIGMA_MAX_PARTS partials (scratch size)
  int csplit = 1;
  if (nb < 2048 && cin > 1) csplit = std::min<long>(cin, std::max<long>(1, std::min<long>(2048, SIGMA_MAX_PARTS) / nb));
  const int cchunk = (cin + csplit - 1) / csplit;
  csplit = (cin + cchunk - 1) / cchunk;
  double* part = reinterpret_cast<double*>(scratch);
  hipLaunchKernelGGL(sigma_partial_kernel, dim3(nb, csplit), dim3(256), 0, s, W, u, v, cout, cin, ks, H, Wd, cchunk,
                     part);
  INF_CHECK_LAUNCH();
  hipLaunchKernelGGL(sigma_final_kernel, dim3(1), dim3(256), 0, s, part, nb * csplit, coeff, factor_out);
  INF_CHECK_LAUNCH();
  return INF_OK;
}

__global__ void pack_kernel(const float* W, const float* factor, float* dst, int cout, int cin, int ks, int Mpad,
                            int Kpad, int mode, int frag) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)Mpad * Kpad) return;
  int m, k;
  if (frag) {   // i = ((rb * nkt + kt) * 64 + lane) * 8 + kk  ->  (32 rb + lane&31, 16 kt + 8 (lane>>5) + kk)
    const int nkt = Kpad / 16;
    const int kk = i & 7, lane = (i >> 3) & 63;
    const long tile = i >> 9;
    const int kt = tile % nkt, rb = tile / nkt;
    m = rb * 32 + (lane & 31);
    k = kt * 16 + 8 * (lane >> 5) + kk;
  } else {
    m = i / Kpad;
    k = i - (long)m * Kpad;
  }
  const float f = factor[0];
  const int kk = ks * ks;
  int co = -1, ci = -1, t = 0;
  switch (mode) {
    case PK_ROWMAJOR: if (m < cout && k < cin) { co = m; ci = k; } break;
    case PK_TRANSPOSE: if (m < cin && k < cout) { co = k; ci = m; } break;
    case PK_IM2COL_FWD: if (m < cout && k < cin * kk) { co = m; ci = k / kk; t = k % kk; } break;
    case PK_IM2COL_BWD: if (m < cin && k < cout * kk) { ci = m; co = k / kk; t = kk - 1 - k % kk; } break;
    case PK_TAPS_FWD: if (m < cout * kk && k < cin) { co = m / kk; t = m % kk; ci = k; } break;
    case PK_TAPS_BWD: if (m < cin * kk && k < cout) { ci = m / kk; t = kk - 1 - m % kk; co = k; } break;
  }
  dst[i] = co >= 0 ? W[((long)co * cin + ci) * kk + t] / f : 0.f;
}
int launch_pack(const float* W, const float* factor, float* dst, int cout, int cin, int ks, int Mpad, int Kpad,
                int mode, hipStream_t s, int frag) {
  const long n = (long)Mpad * Kpad;
  hipLaunchKernelGGL(pack_kernel, dim3((n + 255) / 256), dim3(256), 0, s, W, factor, dst, cout, cin, ks, Mpad, Kpad,
                     mode, frag);
  INF_CHECK_LAUNCH();
  return INF_OK;
}

// Exact three-way bf16 split by truncation: hi = top 16 bits of x, r = x - hi (exact), mid = top 16
// bits of r, lo = r - mid (at most 8 significant bits, so exact in bf16).  hi + mid + lo == x for every
// finite x whose pieces stay in the normal range.
__global__ void split3_kernel(const float* src, uint16_t* dst, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float x = src[i];
  const unsigned u = __float_as_uint(x);
  const float r = x - __uint_as_float(u & 0xffff0000u);
  const unsigned v = __float_as_uint(r);
  const float l = r - __uint_as_float(v & 0xffff0000u);
  const long tile = i >> 9, w = i & 511;
  dst[(tile * 3 + 0) * 512 + w] = (uint16_t)(u >> 16);
  dst[(tile * 3 + 1) * 512 + w] = (uint16_t)(v >> 16);
  dst[(tile * 3 + 2) * 512 + w] = (uint16_t)(__float_as_uint(l) >> 16);
}
int launch_split3(const float* src, uint16_t* dst, long n, hipStream_t s) {
  hipLaunchKernelGGL(split3_kernel, dim3((n + 255) / 256), dim3(256), 0, s, src, dst, n);
  INF_CHECK_LAUNCH();
  return INF_OK;
}

// *exp_out = h3_scale_exp(max |src|) over the whole operand: block maxima folded with atomicMax on the bit patterns
// (non-negative floats order as their bits; NaNs are dropped by fmaxf as before), then one thread converts.  (One
// workgroup per operand took ~50 us for a 512x512 matrix, ~3.6 ms per refresh of the CIFAR model's 12 nets.)
__global__ __launch_bounds__(256) void amax_part_kernel(const float* src, long n, unsigned* mbits) {
  __shared__ float red[4];
  float m = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) m = fmaxf(m, fabsf(src[i]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float r = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    atomicMax(mbits, __float_as_uint(r));
  }
}
__global__ void amax_exp_kernel(int* exp_inout) {
  *exp_inout = h3_scale_exp(__uint_as_float((unsigned)*exp_inout));
}
// Two scaled fp16 pieces per element (common.h split2h): h = rne16(x 2^s), l = rne16(x 2^s - h).
__global__ void split2h_kernel(const float* src, uint16_t* dst, long n, const int* exp) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float S = ldexpf(1.f, *exp);
  const float x = src[i];
  const _Float16 h = (_Float16)(x * S);
  const _Float16 l = (_Float16)__builtin_fmaf(x, S, -(float)h);
  const long tile = i >> 9, w = i & 511;
  dst[(tile * 2 + 0) * 512 + w] = __builtin_bit_cast(uint16_t, h);
  dst[(tile * 2 + 1) * 512 + w] = __builtin_bit_cast(uint16_t, l);
}
int launch_amax_exp(const float* src, long n, int* exp_out, hipStream_t s) {
  INF_HIP(hipMemsetAsync(exp_out, 0, sizeof(int), s));
  const long nb = std::min<long>(256, (n + 4095) / 4096);
  hipLaunchKernelGGL(amax_part_kernel, dim3((unsigned)std::max<long>(nb, 1)), dim3(256), 0, s, src, n,
                     reinterpret_cast<unsigned*>(exp_out));
  hipLaunchKernelGGL(amax_exp_kernel, dim3(1), dim3(1), 0, s, exp_out);
  INF_CHECK_LAUNCH();
  return INF_OK;
}
int launch_split2h(const float* src, uint16_t* dst, long n, int* exp_out, hipStream_t s) {
  INF_TRY(launch_amax_exp(src, n, exp_out, s));
  hipLaunchKernelGGL(split2h_kernel, dim3((n + 255) / 256), dim3(256), 0, s, src, dst, n, (const int*)exp_out);
  INF_CHECK_LAUNCH();
  return INF_OK;
}

__global__ void permute_k23_kernel(const uint16_t* src, uint16_t* dst, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const long base = i & ~511L;                     // (tile, plane) block of 64 lanes x 8 halves
  const int w = (int)(i & 511), L = w >> 3, s = w & 7;
  const int li = L & 31, lh = L >> 5, a = s >> 2, q = s & 3;
  dst[i] = src[base + (li + 32 * a) * 8 + 4 * lh + q];
}
int launch_permute_k23(const uint16_t* src, uint16_t* dst, long ntiles, hipStream_t s) {
  const long n = ntiles * 1024;
  hipLaunchKernelGGL(permute_k23_kernel, dim3((n + 255) / 256), dim3(256), 0, s, src, dst, n);
  INF_CHECK_LAUNCH();
  return INF_OK;
}

}  // namespace inf
