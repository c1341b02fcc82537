// What is left of libinflow's host side once the plans, chains, solvers, estimators and gradient chains have their own
// files (engine.h lists them): the per-thread last-error and launch-profiling state, shutdown, the flow-glue wrappers
// and the debug entries of include/inflow.h.
//
// Reference mapping:
//   inf_logit_forward     <- LogitTransform.forward               (lib/layers/elemwise.py)
//   inf_actnorm_forward   <- ActNorm2d.forward                    (lib/layers/act_norm.py)
//   inf_squeeze2          <- SqueezeLayer(2).forward              (lib/layers/squeeze.py)
//   inf_normal_logprob    <- standard_normal_logprob, summed      (train_img.py)
//   inf_rademacher        <- the Hutchinson probes                (implicit_block.py:297-298)
#include "engine.h"

namespace inf {
static thread_local int g_last_hip = 0;
void set_hip_error(hipError_t e) { g_last_hip = (int)e; }

// ---- opt-in launch timing (per host thread: a profile session records the launches its own thread makes) ----
struct ProfSlot {
  hipEvent_t a, b;
  int tag;
  double flops, bytes, peak_ms;
};
static thread_local std::vector<ProfSlot> g_prof;
static thread_local size_t g_prof_used = 0;
static thread_local bool g_prof_on = false;
bool prof_enabled() { return g_prof_on && g_prof_used < g_prof.size(); }
void prof_begin_launch(hipStream_t s) { (void)hipEventRecord(g_prof[g_prof_used].a, s); }
void prof_end_launch(hipStream_t s, int tag, double flops, double bytes, double peak_ms) {
  ProfSlot& p = g_prof[g_prof_used++];
  (void)hipEventRecord(p.b, s);
  p.tag = tag;
  p.flops = flops;
  p.bytes = bytes;
  p.peak_ms = peak_ms;
}
}  // namespace inf

using namespace inf;

extern "C" {

int inf_version(void) { return 1; }

const char* inf_status_string(int s) {
  switch (s) {
    case INF_OK: return "ok";
    case INF_ERR_INVALID: return "invalid argument";
    case INF_ERR_HIP: return "HIP runtime error";
    case INF_ERR_WORKSPACE: return "workspace too small";
    case INF_ERR_UNSUPPORTED: return "unsupported net layout";
    default: return "unknown status";
  }
}

int inf_last_hip_error(void) { return inf::g_last_hip; }

// ---- teardown ---------------------------------------------------------------------------------
// The calling thread's engine-held host resources: the pinned readback slots and their events, the block kernel's
// statistics buffer and event, the side streams and their fork / join events, the profiling events.  They were kept
// for the process lifetime and left to the HIP runtime's own exit-time teardown; releasing them before it (lib/_hip
// registers this with atexit) leaves that teardown nothing of ours.  Waits for the device first.  Idempotent; nets stay
// valid and the next call re-creates what it needs.
int inf_shutdown(void) {
  int rc = INF_OK;
  if (hipDeviceSynchronize() != hipSuccess) rc = INF_ERR_HIP;
  solve_release_thread();
  logdet_release_thread();
  for (auto& p : g_prof) {
    (void)hipEventDestroy(p.a);
    (void)hipEventDestroy(p.b);
  }
  g_prof.clear();
  g_prof_used = 0;
  g_prof_on = false;
  return rc;
}

// ---- launch timing --------------------------------------------------------------------------
int inf_profile_begin(int max_launches) {
  if (max_launches <= 0) return INF_ERR_INVALID;
  for (auto& p : g_prof) {
    (void)hipEventDestroy(p.a);
    (void)hipEventDestroy(p.b);
  }
  g_prof.assign((size_t)max_launches, ProfSlot{});
  for (auto& p : g_prof) {
    INF_HIP(hipEventCreateWithFlags(&p.a, INF_EV_TIMING));
    INF_HIP(hipEventCreateWithFlags(&p.b, INF_EV_TIMING));
  }
  g_prof_used = 0;
  g_prof_on = true;
  return INF_OK;
}

int inf_profile_end(InfKernelStat* out, int max_out, int* n_out) {
  g_prof_on = false;
  std::vector<InfKernelStat> agg;
  for (size_t i = 0; i < g_prof_used; ++i) {
    ProfSlot& p = g_prof[i];
    INF_HIP(hipEventSynchronize(p.b));
    float ms = 0.f;
    INF_HIP(hipEventElapsedTime(&ms, p.a, p.b));
    InfKernelStat* st = nullptr;
    for (auto& s : agg)
      if (s.tag == p.tag) st = &s;
    if (!st) {
      InfKernelStat z;
      memset(&z, 0, sizeof(z));
      z.tag = p.tag;
      agg.push_back(z);
      st = &agg.back();
    }
    st->launches += 1;
    st->total_ms += ms;
    st->flops += p.flops;
    st->bytes += p.bytes;
    st->peak_ms += p.peak_ms;
  }
  const int n = (int)std::min<size_t>(agg.size(), (size_t)std::max(max_out, 0));
  for (int i = 0; i < n; ++i) out[i] = agg[i];
  if (n_out) *n_out = (int)agg.size();
  g_prof_used = 0;
  return INF_OK;
}

// ---- flow glue ------------------------------------------------------------------------------
int inf_logit_forward(const float* x, float* y, const float* logp_in, float* logp_out, int B, int per, float alpha,
                      void* stream) {
  if (!x || !y || !logp_out || B <= 0 || per <= 0) return INF_ERR_INVALID;
  return glue_logit(x, y, logp_in, logp_out, B, per, alpha, (hipStream_t)stream);
}
int inf_actnorm_forward(const float* x, float* y, const float* w, const float* b, const float* logp_in,
                        float* logp_out, int B, int C, int hw, void* stream) {
  if (!x || !y || !w || !b || B <= 0) return INF_ERR_INVALID;
  return glue_actnorm(x, y, w, b, logp_in, logp_out, B, C, hw, (hipStream_t)stream);
}
int inf_squeeze2(const float* x, float* y, int B, int C, int H, int W, void* stream) {
  if (!x || !y || B <= 0 || (H & 1) || (W & 1)) return INF_ERR_INVALID;
  return glue_squeeze2(x, y, B, C, H, W, (hipStream_t)stream);
}
int inf_normal_logprob(const float* z, float* out, int B, int per, void* stream) {
  if (!z || !out || B <= 0) return INF_ERR_INVALID;
  return glue_normal_logprob(z, out, B, per, (hipStream_t)stream);
}
int inf_rademacher(float* out, size_t n, uint64_t seed, uint64_t offset, void* stream) {
  if (!out && n) return INF_ERR_INVALID;
  return glue_rademacher(out, n, seed, offset, (hipStream_t)stream);
}

int inf_net313_kernel_family(int hidden, int channels, int height, int width, int batch, int nnets, int layout_nets,
                             int k128_policy, int mode, int f16x3) {
  if (hidden <= 0 || channels <= 0 || height <= 0 || width <= 0 || k128_policy < 0 || k128_policy > 3 ||
      mode < MODE_EVAL || mode > MODE_EVALSAVE)
    return -INF_ERR_INVALID;
  const int fam = net313_family(hidden, channels, height, width, batch, nnets, layout_nets, k128_policy, mode, f16x3 != 0);
  return fam < 0 ? -INF_ERR_UNSUPPORTED : fam;
}

int inf_series_group(int hidden, int channels, int height, int width, int batch, int nnets, int concurrent,
                     int k128_policy, int f16x3) {
  if (hidden <= 0 || channels <= 0 || height <= 0 || width <= 0 || batch <= 0 || nnets < 1 || nnets > 2 ||
      concurrent < 1 || k128_policy < 0 || k128_policy > 3)
    return -INF_ERR_INVALID;
  if (net313_family(hidden, channels, height, width, batch, nnets, nnets, k128_policy, MODE_VJP, f16x3 != 0) < 0)
    return -INF_ERR_UNSUPPORTED;
  return net313_series_group(hidden, channels, height, width, batch, nnets, concurrent, k128_policy, f16x3 != 0);
}

// ---- debug entries ----------------------------------------------------------------------------
int inf_debug_poison_lds(void* stream) { return glue_poison_lds((hipStream_t)stream); }

// readback contract check (inflow.h): round r writes base_r + i (i < n) into a pinned coherent slot, once from a kernel
// whose launch completes the slot's event (the zero-copy Broyden sums) and once through a device buffer and a D2H copy
// followed by a recorded event (the reduction + copy form); the host waits with host_wait and compares every value
__global__ void readback_pattern_kernel(double* out, int n, double base) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = base + (double)i;
}
int inf_debug_readback_check(int iters, int n, void* stream) {
  if (iters < 0 || n <= 0 || n > (1 << 20)) return -INF_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  double* host = nullptr;
  double* dev = nullptr;
  hipEvent_t ev = nullptr;
  int bad = 0, rc = INF_OK;
  if (hipHostMalloc(reinterpret_cast<void**>(&host), sizeof(double) * n, hipHostMallocCoherent) != hipSuccess ||
      hipMalloc(reinterpret_cast<void**>(&dev), sizeof(double) * n) != hipSuccess ||
      hipEventCreateWithFlags(&ev, INF_EV_SYNC) != hipSuccess) {
    rc = INF_ERR_HIP;
  }
  const dim3 grid((n + 255) / 256), blk(256);
  for (int r = 0; r < iters && rc == INF_OK; ++r) {
    for (int form = 0; form < 2 && rc == INF_OK; ++form) {
      const double base = 1e6 * (2 * r + form + 1);
      if (form == 0) {
        hipExtLaunchKernelGGL(readback_pattern_kernel, grid, blk, 0, s, nullptr, ev, 0, host, n, base);
      } else {
        hipLaunchKernelGGL(readback_pattern_kernel, grid, blk, 0, s, dev, n, base);
        if (hipMemcpyAsync(host, dev, sizeof(double) * n, hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipEventRecord(ev, s) != hipSuccess) rc = INF_ERR_HIP;
      }
      if (hipGetLastError() != hipSuccess) rc = INF_ERR_HIP;
      if (rc == INF_OK) rc = host_wait(ev);
      for (int i = 0; i < n && rc == INF_OK; ++i) bad += host[i] != base + (double)i;
    }
  }
  (void)hipStreamSynchronize(s);
  if (ev) (void)hipEventDestroy(ev);
  if (dev) (void)hipFree(dev);
  if (host) (void)hipHostFree(host);
  return rc == INF_OK ? bad : -rc;
}

}  // extern "C"
