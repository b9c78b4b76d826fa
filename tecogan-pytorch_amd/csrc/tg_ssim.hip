// The two frame metrics of the official evaluation protocol (codes/official_metrics/metrics.py:60-73) that the
// in-loop MetricCalculator does not have, for gfx950: SSIM and PSNR on the UNROUNDED Y plane of uint8 HWC frames,
// both on a crop window given by arguments (the protocol crops twice; neither crop needs a copy).
//
//   Y = 16 + (65.481 R + 128.553 G + 24.966 B) / 255 = 16 + y' / 255000,   y' = 65481 R + 128553 G + 24966 B,
// an integer of at most 55 845 000 < 2^26.  Everything up to the last few operations is therefore exact integer
// arithmetic, and the results are bit-identical from run to run, for any batch split and for a windowed call vs a
// call on a contiguous copy of the window (tiles are laid out from the window's origin).
//
// SSIM (skimage.measure.compare_ssim defaults: 7x7 uniform window, sample covariance, K1 0.01, K2 0.03, mean over
// the positions whose window lies inside the image; data_range = max - min of the PREDICTED frame's Y):
//   ssim_range_kernel   min / max of y' of the predicted frame over the window (integer atomics: order-independent)
//   ssim_tile_kernel    one workgroup per (frame, 16 x 64 tile of window positions): y' of both frames for the tile
//                       plus a 6-pixel apron in LDS, 7-sums along rows of x, y (u32) and xx, yy, xy (u64) in LDS,
//                       7-sums along columns per position, then with S the 49-term sums
//                         vx = (49 Sxx - Sx^2) / (49 * 48 * 255000^2)   (the centred moment is < 7.49e18: fits int64)
//                         ux = Sx / (49 * 255000) + 16
//                       and the SSIM formula in fp64; fixed-order reduction to one fp64 partial per workgroup
//   ssim_final_kernel   per frame: partials summed in index order / positions
// A constant predicted frame has data_range 0, so C1 = C2 = 0 and flat positions give 0/0: the frame's value is
// NaN, as numpy's is.
//
// PSNR: psnr_yfloat_kernel writes, per (frame, block of 4096 window pixels), the exact sum of (y'_true - y'_pred)^2
// as a 64-bit integer (one term is at most 3.12e15, so a partial stays below 2^64 up to 5900 pixels); the caller
// adds the partials and applies 255000^-2.
#include "tg_common.h"

namespace tg {
namespace {

constexpr int SS_TH = 16;                 // tile: window positions per workgroup
constexpr int SS_TW = 64;
constexpr int SS_WIN = 7;
constexpr int SS_IH = SS_TH + SS_WIN - 1;  // staged rows / columns
constexpr int SS_IW = SS_TW + SS_WIN - 1;
constexpr int SS_THREADS = 256;
constexpr int PS_PIX = 4096;              // pixels per PSNR partial (< 5900, see above)

__device__ __forceinline__ unsigned yprime(const uint8_t* __restrict__ p) {
  return 65481u * p[0] + 128553u * p[1] + 24966u * p[2];
}

struct SsimArgs {
  const uint8_t* a;    // true frames (frames, ah, aw, 3)
  const uint8_t* b;    // predicted frames (frames, bh, bw, 3)
  int ah, aw, bh, bw;  // full frames
  int y0, x0, h, w;    // window
};

__global__ __launch_bounds__(64) void ssim_range_init_kernel(unsigned* __restrict__ range, int frames) {
  const int f = blockIdx.x * 64 + threadIdx.x;
  if (f < frames) {
    range[2 * f] = 0xFFFFFFFFu;
    range[2 * f + 1] = 0u;
  }
}

__global__ __launch_bounds__(256) void ssim_range_kernel(SsimArgs s, unsigned* __restrict__ range) {
  __shared__ unsigned smin[4], smax[4];
  const int f = blockIdx.y;
  const uint8_t* pb = s.b + (long long)f * s.bh * s.bw * 3;
  const long long hw = (long long)s.h * s.w;
  unsigned lo = 0xFFFFFFFFu, hi = 0u;
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < hw;
       p += (long long)gridDim.x * blockDim.x) {
    const int r = (int)(p / s.w), c = (int)(p - (long long)r * s.w);
    const unsigned v = yprime(pb + ((long long)(s.y0 + r) * s.bw + (s.x0 + c)) * 3);
    lo = v < lo ? v : lo;
    hi = v > hi ? v : hi;
  }
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned l2 = __shfl_down(lo, o, 64), h2 = __shfl_down(hi, o, 64);
    lo = l2 < lo ? l2 : lo;
    hi = h2 > hi ? h2 : hi;
  }
  if ((threadIdx.x & 63) == 0) {
    smin[threadIdx.x >> 6] = lo;
    smax[threadIdx.x >> 6] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < 4; ++i) {
      lo = smin[i] < lo ? smin[i] : lo;
      hi = smax[i] > hi ? smax[i] : hi;
    }
    atomicMin(range + 2 * f, lo);
    atomicMax(range + 2 * f + 1, hi);
  }
}

__global__ __launch_bounds__(SS_THREADS) void ssim_tile_kernel(SsimArgs s, const unsigned* __restrict__ range,
                                                               double* __restrict__ part) {
  __shared__ unsigned xs[SS_IH * SS_IW], ys[SS_IH * SS_IW];
  __shared__ unsigned hx[SS_IH * SS_TW], hy[SS_IH * SS_TW];
  __shared__ unsigned long long hxx[SS_IH * SS_TW], hyy[SS_IH * SS_TW], hxy[SS_IH * SS_TW];
  __shared__ double red[SS_THREADS / 64];
  const int tid = threadIdx.x;
  const int f = blockIdx.z;
  const int r0 = blockIdx.y * SS_TH, c0 = blockIdx.x * SS_TW;      // tile origin inside the window
  const uint8_t* pa = s.a + (long long)f * s.ah * s.aw * 3;
  const uint8_t* pb = s.b + (long long)f * s.bh * s.bw * 3;

  // y' of the tile + apron; outside the window: 0 (such pixels only reach positions that are masked below)
  for (int i = tid; i < SS_IH * SS_IW; i += SS_THREADS) {
    const int r = r0 + i / SS_IW, c = c0 + i % SS_IW;
    unsigned va = 0u, vb = 0u;
    if (r < s.h && c < s.w) {
      va = yprime(pa + ((long long)(s.y0 + r) * s.aw + (s.x0 + c)) * 3);
      vb = yprime(pb + ((long long)(s.y0 + r) * s.bw + (s.x0 + c)) * 3);
    }
    xs[i] = va;
    ys[i] = vb;
  }
  __syncthreads();

  // 7-sums along rows
  for (int i = tid; i < SS_IH * SS_TW; i += SS_THREADS) {
    const int r = i / SS_TW, c = i % SS_TW;
    unsigned sx = 0u, sy = 0u;
    unsigned long long sxx = 0ull, syy = 0ull, sxy = 0ull;
#pragma unroll
    for (int k = 0; k < SS_WIN; ++k) {
      const unsigned long long x = xs[r * SS_IW + c + k], y = ys[r * SS_IW + c + k];
      sx += (unsigned)x;
      sy += (unsigned)y;
      sxx += x * x;
      syy += y * y;
      sxy += x * y;
    }
    hx[i] = sx; hy[i] = sy; hxx[i] = sxx; hyy[i] = syy; hxy[i] = sxy;
  }
  __syncthreads();

  // data_range of the predicted frame -> C1, C2
  const double R = (double)(range[2 * f + 1] - range[2 * f]) / 255000.0;
  const double C1 = (0.01 * R) * (0.01 * R), C2 = (0.03 * R) * (0.03 * R);
  const int oh = s.h - (SS_WIN - 1), ow = s.w - (SS_WIN - 1);      // valid positions
  const int c = tid % SS_TW;
  double acc = 0.0;
  for (int j = 0; j < SS_TH / (SS_THREADS / SS_TW); ++j) {
    const int r = (tid / SS_TW) * (SS_TH / (SS_THREADS / SS_TW)) + j;
    unsigned sx = 0u, sy = 0u;
    unsigned long long sxx = 0ull, syy = 0ull, sxy = 0ull;
#pragma unroll
    for (int k = 0; k < SS_WIN; ++k) {
      const int i = (r + k) * SS_TW + c;
      sx += hx[i]; sy += hy[i]; sxx += hxx[i]; syy += hyy[i]; sxy += hxy[i];
    }
    if (r0 + r < oh && c0 + c < ow) {
      const long long lx = (long long)sx, ly = (long long)sy;
      const long long mxx = 49ll * (long long)sxx - lx * lx;
      const long long myy = 49ll * (long long)syy - ly * ly;
      const long long mxy = 49ll * (long long)sxy - lx * ly;
      const double D = 49.0 * 48.0 * 255000.0 * 255000.0;           // exact
      const double vx = (double)mxx / D, vy = (double)myy / D, vxy = (double)mxy / D;
      const double ux = (double)lx / (49.0 * 255000.0) + 16.0, uy = (double)ly / (49.0 * 255000.0) + 16.0;
      const double A1 = 2.0 * ux * uy + C1, A2 = 2.0 * vxy + C2;
      const double B1 = ux * ux + uy * uy + C1, B2 = vx + vy + C2;
      acc += (A1 * A2) / (B1 * B2);
    }
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    const int nb = gridDim.x * gridDim.y;
    part[(long long)f * nb + blockIdx.y * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
  }
}

__global__ __launch_bounds__(64) void ssim_final_kernel(const double* __restrict__ part, int nb, int frames,
                                                        double count, double* __restrict__ ssim) {
  const int f = blockIdx.x * 64 + threadIdx.x;
  if (f >= frames) return;
  double t = 0.0;
  for (int i = 0; i < nb; ++i) t += part[(long long)f * nb + i];
  ssim[f] = t / count;
}

__global__ __launch_bounds__(256) void psnr_yfloat_kernel(SsimArgs s, unsigned long long* __restrict__ part) {
  __shared__ unsigned long long sm[4];
  const int f = blockIdx.y;
  const uint8_t* pa = s.a + (long long)f * s.ah * s.aw * 3;
  const uint8_t* pb = s.b + (long long)f * s.bh * s.bw * 3;
  const long long hw = (long long)s.h * s.w;
  const long long p0 = (long long)blockIdx.x * PS_PIX;
  unsigned long long t = 0ull;
  for (int k = threadIdx.x; k < PS_PIX; k += 256) {
    const long long p = p0 + k;
    if (p < hw) {
      const int r = (int)(p / s.w), c = (int)(p - (long long)r * s.w);
      const long long d = (long long)yprime(pa + ((long long)(s.y0 + r) * s.aw + (s.x0 + c)) * 3) -
                          (long long)yprime(pb + ((long long)(s.y0 + r) * s.bw + (s.x0 + c)) * 3);
      t += (unsigned long long)(d * d);
    }
  }
  for (int o = 32; o > 0; o >>= 1) t += __shfl_down(t, o, 64);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = t;
  __syncthreads();
  if (threadIdx.x == 0) part[(long long)f * gridDim.x + blockIdx.x] = sm[0] + sm[1] + sm[2] + sm[3];
}

inline int ssim_blocks(int h, int w) {
  return cdiv(h - (SS_WIN - 1), SS_TH) * cdiv(w - (SS_WIN - 1), SS_TW);
}

// the window must lie inside both frames; sizes bounded so that byte offsets of a batch stay far below 2^63
inline bool window_ok(int frames, int th, int tw, int ph, int pw, int y0, int x0, int h, int w) {
  return frames > 0 && frames <= 65535 && th > 0 && tw > 0 && ph > 0 && pw > 0 && th <= 32768 && tw <= 32768 &&
         ph <= 32768 && pw <= 32768 && y0 >= 0 && x0 >= 0 && h > 0 && w > 0 && y0 <= th - h && y0 <= ph - h &&
         x0 <= tw - w && x0 <= pw - w;
}

}  // namespace
}  // namespace tg

using namespace tg;

extern "C" int64_t tg_ssim_workspace_bytes(int frames, int h, int w) {
  if (frames <= 0 || h < SS_WIN || w < SS_WIN || h > 32768 || w > 32768) return -1;
  return (int64_t)frames * 8 + (int64_t)frames * ssim_blocks(h, w) * (int64_t)sizeof(double);
}

extern "C" int tg_ssim_y_u8(const uint8_t* true_hwc, const uint8_t* pred_hwc, int frames, int true_h, int true_w,
                            int pred_h, int pred_w, int y0, int x0, int h, int w, double* ssim, void* workspace,
                            size_t workspace_bytes, tg_stream_t stream) {
  TG_REQUIRE(true_hwc && pred_hwc && ssim && workspace, TG_E_ARG, "ssim_y_u8: null pointer");
  TG_REQUIRE(window_ok(frames, true_h, true_w, pred_h, pred_w, y0, x0, h, w), TG_E_SHAPE,
             "ssim_y_u8: frames=%d true %dx%d pred %dx%d window (%d,%d) %dx%d does not lie inside both frames",
             frames, true_h, true_w, pred_h, pred_w, y0, x0, h, w);
  TG_REQUIRE(h >= SS_WIN && w >= SS_WIN, TG_E_SHAPE, "ssim_y_u8: the window (%dx%d) is smaller than 7x7", h, w);
  const int64_t need = tg_ssim_workspace_bytes(frames, h, w);
  TG_REQUIRE(need > 0 && workspace_bytes >= (size_t)need, TG_E_ARG, "ssim_y_u8: workspace of %zu bytes, %lld needed",
             workspace_bytes, (long long)need);
  SsimArgs s{true_hwc, pred_hwc, true_h, true_w, pred_h, pred_w, y0, x0, h, w};
  unsigned* range = (unsigned*)workspace;
  double* part = (double*)((char*)workspace + (size_t)frames * 8);
  const int gx = cdiv(w - (SS_WIN - 1), SS_TW), gy = cdiv(h - (SS_WIN - 1), SS_TH);
  TG_REQUIRE(gy <= 65535, TG_E_SHAPE, "ssim_y_u8: window too tall (%d)", h);
  hipLaunchKernelGGL(ssim_range_init_kernel, dim3(cdiv(frames, 64)), dim3(64), 0, (hipStream_t)stream, range,
                     frames);
  int rc = check_launch("ssim_range_init");
  if (rc != TG_OK) return rc;
  long long bx = ((long long)h * w + 1023) / 1024;
  hipLaunchKernelGGL(ssim_range_kernel, dim3((unsigned)(bx > 256 ? 256 : bx), frames), dim3(256), 0,
                     (hipStream_t)stream, s, range);
  rc = check_launch("ssim_range");
  if (rc != TG_OK) return rc;
  hipLaunchKernelGGL(ssim_tile_kernel, dim3(gx, gy, frames), dim3(SS_THREADS), 0, (hipStream_t)stream, s,
                     (const unsigned*)range, part);
  rc = check_launch("ssim_tile");
  if (rc != TG_OK) return rc;
  hipLaunchKernelGGL(ssim_final_kernel, dim3(cdiv(frames, 64)), dim3(64), 0, (hipStream_t)stream,
                     (const double*)part, gx * gy, frames,
                     (double)(h - (SS_WIN - 1)) * (double)(w - (SS_WIN - 1)), ssim);
  return check_launch("ssim_final");
}

extern "C" int64_t tg_psnr_yfloat_partials(int h, int w) {
  if (h <= 0 || w <= 0 || h > 32768 || w > 32768) return -1;
  return ((int64_t)h * w + PS_PIX - 1) / PS_PIX;
}

extern "C" int tg_psnr_yfloat_sse_u8(const uint8_t* true_hwc, const uint8_t* pred_hwc, int frames, int true_h,
                                     int true_w, int pred_h, int pred_w, int y0, int x0, int h, int w,
                                     uint64_t* partials, tg_stream_t stream) {
  TG_REQUIRE(true_hwc && pred_hwc && partials, TG_E_ARG, "psnr_yfloat_sse_u8: null pointer");
  TG_REQUIRE(window_ok(frames, true_h, true_w, pred_h, pred_w, y0, x0, h, w), TG_E_SHAPE,
             "psnr_yfloat_sse_u8: frames=%d true %dx%d pred %dx%d window (%d,%d) %dx%d does not lie inside both "
             "frames", frames, true_h, true_w, pred_h, pred_w, y0, x0, h, w);
  SsimArgs s{true_hwc, pred_hwc, true_h, true_w, pred_h, pred_w, y0, x0, h, w};
  const int64_t nb = tg_psnr_yfloat_partials(h, w);
  hipLaunchKernelGGL(psnr_yfloat_kernel, dim3((unsigned)nb, frames), dim3(256), 0, (hipStream_t)stream, s,
                     (unsigned long long*)partials);
  return check_launch("psnr_yfloat_sse_u8");
}
