// Scene cuts of infer_stream, decided on the device.
//
//   tg_scene_cut_flags: per pair of consecutive LR frames the sum of absolute luma differences and the L1 distance of the
//     two 32-bin luma histograms, both in exact integers, compared with two thresholds on the device: one int32 flag per
//     frame.  The formula is the specification (include/tecogan_hip.h); tests/scene_cut_ref.py restates it in numpy.
//   tg_zero_if_flag: the reset itself -- a fill that every thread leaves at once unless the flag is set.  The stream
//     issues one per frame in front of tg_frnet_step_srnet; the host never learns the flag before the batch is retired.
//
// All three kernels are streaming or launch-bound and small: an LR frame of 134x320 is 0.5 MB and is read twice (as the
// later and as the earlier frame of a pair); the fill writes the 8.2 MB HR state only at a cut.
#include "tg_common.h"

namespace tg {

constexpr int SC_BINS = 32;
constexpr int SC_THREADS = 256;
constexpr int SC_WAVES = SC_THREADS / 64;
constexpr long long SC_MAX_PIXELS = 1LL << 28;  // per-thread SAD partials stay far below 2^32, 2N fits hdist's 32 bits

// clamp(floor(fma(x, 255, 0.5)), 0, 255), NaN -> 0: both comparisons are false for a NaN
__device__ __forceinline__ int quant255(float x) {
  float v = floorf(__fmaf_rn(x, 255.f, 0.5f));
  v = v >= 0.f ? v : 0.f;
  v = v > 255.f ? 255.f : v;
  return (int)v;
}
__device__ __forceinline__ int luma8(float r, float g, float b) {
  return (77 * quant255(r) + 150 * quant255(g) + 29 * quant255(b) + 128) >> 8;
}

// block (bx, f): pixels bx*256 + tid, + gridDim.x*256, ... (in units of V pixels) of frame f -- its histogram, and for
// f >= 1 the absolute differences against frame f - 1.  V = 4: every plane of every frame is 16-byte aligned.
// ws: [n] u64 SAD, then [(n + 1) x 32] u32 histograms, zeroed before the launch.
template <int V>
__global__ __launch_bounds__(SC_THREADS) void scene_stats_kernel(const float* __restrict__ frames, long long plane,
                                                                 unsigned long long* __restrict__ ws_sad,
                                                                 unsigned* __restrict__ ws_hist) {
  __shared__ unsigned hist[SC_WAVES][SC_BINS];
  __shared__ unsigned wave_sad[SC_WAVES];
  const int tid = threadIdx.x, wave = tid >> 6, f = blockIdx.y;
  if (tid < SC_WAVES * SC_BINS) (&hist[0][0])[tid] = 0;
  __syncthreads();
  const float* cur = frames + (long long)f * 3 * plane;
  const float* prev = f > 0 ? cur - 3 * plane : cur;              // read only when f >= 1
  const long long units = plane / V, step = (long long)gridDim.x * SC_THREADS;
  unsigned sad = 0;
  for (long long u = (long long)blockIdx.x * SC_THREADS + tid; u < units; u += step) {
    float c[3][V], p[3][V];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      if constexpr (V == 4) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(cur + ch * plane + 4 * u);
        c[ch][0] = t[0]; c[ch][1] = t[1]; c[ch][2] = t[2]; c[ch][3] = t[3];
        if (f > 0) {
          const f32x4 s = *reinterpret_cast<const f32x4*>(prev + ch * plane + 4 * u);
          p[ch][0] = s[0]; p[ch][1] = s[1]; p[ch][2] = s[2]; p[ch][3] = s[3];
        }
      } else {
        c[ch][0] = cur[ch * plane + u];
        if (f > 0) p[ch][0] = prev[ch * plane + u];
      }
    }
#pragma unroll
    for (int x = 0; x < V; ++x) {
      const int y = luma8(c[0][x], c[1][x], c[2][x]);
      atomicAdd(&hist[wave][y >> 3], 1u);
      if (f > 0) {
        const int d = y - luma8(p[0][x], p[1][x], p[2][x]);
        sad += (unsigned)(d < 0 ? -d : d);
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sad += __shfl_xor(sad, o, 64);
  if ((tid & 63) == 0) wave_sad[wave] = sad;
  __syncthreads();
  if (tid < SC_BINS) {
    unsigned s = 0;
#pragma unroll
    for (int k = 0; k < SC_WAVES; ++k) s += hist[k][tid];
    if (s) atomicAdd(&ws_hist[f * SC_BINS + tid], s);
  }
  if (tid == 0 && f > 0) {
    unsigned long long s = 0;
#pragma unroll
    for (int k = 0; k < SC_WAVES; ++k) s += wave_sad[k];
    if (s) atomicAdd(&ws_sad[f - 1], s);
  }
}

// one workgroup; 32 lanes per pair (a lane per bin), 8 pairs at a time
__global__ __launch_bounds__(SC_THREADS) void scene_decide_kernel(const unsigned long long* __restrict__ ws_sad,
                                                                  const unsigned* __restrict__ ws_hist, int n,
                                                                  unsigned long long s_min, unsigned long long d_min,
                                                                  const uint8_t* __restrict__ forced, int detect,
                                                                  int32_t* __restrict__ flags,
                                                                  unsigned long long* __restrict__ sad,
                                                                  uint32_t* __restrict__ hdist) {
  const int bin = threadIdx.x & (SC_BINS - 1);
  for (int j = threadIdx.x / SC_BINS; j < n; j += SC_THREADS / SC_BINS) {      // (uniform over a group of 32 lanes)
    const unsigned a = ws_hist[(j + 1) * SC_BINS + bin], b = ws_hist[j * SC_BINS + bin];
    unsigned d = a > b ? a - b : b - a;
#pragma unroll
    for (int o = SC_BINS / 2; o > 0; o >>= 1) d += __shfl_xor(d, o, SC_BINS);
    if (bin == 0) {
      const unsigned long long s = ws_sad[j];
      const bool cut = (forced && forced[j]) || (detect && s >= s_min && (unsigned long long)d >= d_min);
      flags[j] = cut ? 1 : 0;
      sad[j] = s;
      hdist[j] = d;
    }
  }
}

// head bytes up to the first 16-byte boundary, 16-byte stores, tail bytes
__global__ __launch_bounds__(256) void zero_if_flag_kernel(uint8_t* __restrict__ dst, long long bytes,
                                                           const int32_t* __restrict__ flag) {
  if (*flag == 0) return;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x, step = (long long)gridDim.x * 256;
  long long head = (long long)((16 - ((uintptr_t)dst & 15)) & 15);
  head = head < bytes ? head : bytes;
  const long long nvec = (bytes - head) >> 4, tail0 = head + (nvec << 4);
  u32x4* body = reinterpret_cast<u32x4*>(dst + head);
  for (long long k = i; k < nvec; k += step) body[k] = u32x4{0u, 0u, 0u, 0u};
  if (i < head) dst[i] = 0;
  if (i < bytes - tail0) dst[tail0 + i] = 0;                      // (fewer than 16 of each: the first threads do them)
}

}  // namespace tg

extern "C" int64_t tg_scene_cut_workspace_bytes(int n) {
  if (n < 1) return 0;
  return (int64_t)n * 8 + (int64_t)(n + 1) * tg::SC_BINS * 4;
}

extern "C" int tg_scene_cut_flags(const float* frames, int n, int h, int w, uint64_t s_min, uint64_t d_min,
                                  const uint8_t* forced, int detect, int32_t* flags, uint64_t* sad, uint32_t* hdist,
                                  void* workspace, int64_t workspace_bytes, tg_stream_t stream) {
  TG_REQUIRE(frames && flags && sad && hdist && workspace, TG_E_ARG, "scene_cut_flags: null pointer");
  TG_REQUIRE(n >= 1 && h >= 1 && w >= 1, TG_E_ARG, "scene_cut_flags: n=%d h=%d w=%d (all >= 1)", n, h, w);
  TG_REQUIRE((uintptr_t)frames % 4 == 0 && (uintptr_t)flags % 4 == 0 && (uintptr_t)sad % 8 == 0 &&
                 (uintptr_t)hdist % 4 == 0 && (uintptr_t)workspace % 8 == 0,
             TG_E_ARG, "scene_cut_flags: misaligned pointer");
  TG_REQUIRE(workspace_bytes >= tg_scene_cut_workspace_bytes(n), TG_E_ARG,
             "scene_cut_flags: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
             (long long)tg_scene_cut_workspace_bytes(n));
  const long long plane = (long long)h * w;
  TG_REQUIRE(plane <= tg::SC_MAX_PIXELS, TG_E_SHAPE, "scene_cut_flags: %lld pixels per frame", plane);
  const hipStream_t st = (hipStream_t)stream;
  unsigned long long* ws_sad = static_cast<unsigned long long*>(workspace);
  unsigned* ws_hist = reinterpret_cast<unsigned*>(ws_sad + n);
  hipError_t e = hipMemsetAsync(workspace, 0, (size_t)tg_scene_cut_workspace_bytes(n), st);
  if (e != hipSuccess) {
    tg::set_error("scene_cut_flags: hipMemsetAsync: %s", hipGetErrorString(e));
    return TG_E_HIP;
  }
  const bool vec = plane % 4 == 0 && (uintptr_t)frames % 16 == 0;
  const long long units = vec ? plane / 4 : plane;
  // about 8 units a thread, at most 1024 workgroups a frame
  long long bpf = (units + 8 * tg::SC_THREADS - 1) / (8 * tg::SC_THREADS);
  bpf = bpf < 1 ? 1 : (bpf > 1024 ? 1024 : bpf);
  const dim3 grid((unsigned)bpf, (unsigned)(n + 1)), block(tg::SC_THREADS);
  if (vec) hipLaunchKernelGGL((tg::scene_stats_kernel<4>), grid, block, 0, st, frames, plane, ws_sad, ws_hist);
  else hipLaunchKernelGGL((tg::scene_stats_kernel<1>), grid, block, 0, st, frames, plane, ws_sad, ws_hist);
  int rc = tg::check_launch("scene_stats");
  if (rc != TG_OK) return rc;
  hipLaunchKernelGGL(tg::scene_decide_kernel, dim3(1), block, 0, st, ws_sad, ws_hist, n, (unsigned long long)s_min,
                     (unsigned long long)d_min, forced, detect, flags, reinterpret_cast<unsigned long long*>(sad),
                     hdist);
  return tg::check_launch("scene_decide");
}

extern "C" int tg_zero_if_flag(void* dst, int64_t bytes, const int32_t* flag, tg_stream_t stream) {
  TG_REQUIRE(dst && flag, TG_E_ARG, "zero_if_flag: null pointer");
  TG_REQUIRE(bytes >= 0 && (uintptr_t)flag % 4 == 0, TG_E_ARG, "zero_if_flag: bytes=%lld, flag %% 4 = %d",
             (long long)bytes, (int)((uintptr_t)flag % 4));
  if (bytes == 0) return TG_OK;
  // about 8 stores of 16 bytes a thread: one workgroup per CU's worth for the 8.2 MB HR state of a 134x320 frame
  long long blocks = (bytes / 16 + 8 * 256 - 1) / (8 * 256);
  blocks = blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks);
  hipLaunchKernelGGL(tg::zero_if_flag_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                     static_cast<uint8_t*>(dst), (long long)bytes, flag);
  return tg::check_launch("zero_if_flag");
}
