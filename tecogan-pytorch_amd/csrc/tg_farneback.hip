// tOF's optical flow for gfx950: dense Farneback flow with the one parameter set both reference call sites use
// (codes/official_metrics/metrics.py:149, codes/metrics/metric_calculator.py:270: pyr_scale 0.5, levels 3, winsize 15,
// iterations 3, poly_n 5, poly_sigma 1.2, flags 0), and the mean end-point error of two flow fields.  The
// specification is DESIGN.md section 7f / tests/farneback_ref.py (a restatement of the published algorithm; it has
// not been compared with OpenCV).
//
// Stages, each ONE launch for all images of a call (blockIdx.z = image; tiles are laid out from the image origin, so
// results do not depend on the batch split, and the top-left h x w of larger frames is read in place):
//   fb_gray_kernel          uint8 RGB -> uint8 gray, (4899 R + 9617 G + 1868 B + 8192) >> 14
//   fb_hblur_kernel         level image 1/2: Gaussian along rows of the full-resolution frame (reflect-101), a row
//                           segment + apron staged in LDS
//   fb_vblur_resize_kernel  level image 2/2: Gaussian along columns at the four bilinear neighbours + the resize
//   fb_polyexp_kernel       polynomial expansion: 16 x 64 tile + 5-pixel apron in LDS, the three vertical 11-tap sums
//                           in LDS, the six horizontal ones from there; R is written as five planes per image
//   fb_update_kernel        per pixel: bilinear gather of R1 at x + flow, the update matrix M (five planes)
//   fb_blur_solve_kernel    15 x 15 box sums of M's five planes through LDS (16 x 64 tile + 7-pixel apron, rows then
//                           columns), the 2 x 2 solve, the new flow
//   fb_resize_flow_kernel   bilinear resize of the previous level's flow, times 2
//   flow_epe_kernel         per image: float32 end-point error per pixel, fp64 partial per thread (fixed stride), fixed
//                           tree over the workgroup
// The 5-float records R and M are kept as planes ((image, 5, h, w)): every load and store of the stencil stages is
// a coalesced row read, and the gather reads 4 neighbours x 5 planes.  Flows are (image, h, w, 2).
//
// Numerics: fp32, sums in the order tests/farneback_ref.py's float32 form (alt32) takes them, and no contraction of
// a * b + c into fused multiply-adds in this file, so the kernels and alt32 round alike.  Filter taps, the inverse
// Gram matrix and the sampling positions of the resizes are computed in fp64 and rounded once.
// No kernel waits for another workgroup; nothing here is atomic.
#include <math.h>

#include "tg_common.h"

#pragma clang fp contract(off)

namespace tg {
namespace {

constexpr int FB_POLY_N = 5;
constexpr int FB_WIN = 15;
constexpr int FB_ITERS = 3;
constexpr int FB_MAX_LEVEL = 3;
constexpr int FB_MIN_SIZE = 32;
constexpr int FB_TH = 16, FB_TW = 64, FB_THREADS = 256;
constexpr int FB_MAX_TAPS = 19;
constexpr int FB_PE_IW = FB_TW + 2 * FB_POLY_N, FB_PE_IH = FB_TH + 2 * FB_POLY_N;
constexpr int FB_BX_IW = FB_TW + FB_WIN - 1, FB_BX_IH = FB_TH + FB_WIN - 1;
constexpr int FB_EPE_THREADS = 1024;

struct BlurTaps {
  float t[FB_MAX_TAPS];
  int n;
};
struct PolyK {
  float g[FB_POLY_N + 1], xg[FB_POLY_N + 1], xxg[FB_POLY_N + 1];
  float ig11, ig03, ig33, ig55;
};

// ---- host-side constants and geometry -------------------------------------------------------------------------
inline int top_level(int h, int w) {
  const int m = h < w ? h : w;
  int k = 0;
  while (k < FB_MAX_LEVEL && (m >> (k + 1)) >= FB_MIN_SIZE) ++k;   // m * 0.5^(k+1) >= 32  <=>  floor(m / 2^(k+1)) >= 32
  return k;
}
inline int level_dim(int n, int k) {      // rint(n / 2^k), half to even
  if (k == 0) return n;
  int q = n >> k;
  const int rem = n & ((1 << k) - 1), half = 1 << (k - 1);
  if (rem > half || (rem == half && (q & 1))) ++q;
  return q;
}
inline BlurTaps blur_taps(int k) {
  BlurTaps b{};
  const double sigma = ((double)(1 << k) - 1.0) * 0.5;
  int n = (int)nearbyint(5.0 * sigma) | 1;
  b.n = n < 3 ? 3 : n;
  if (k == 0) {
    b.t[0] = 0.25f; b.t[1] = 0.5f; b.t[2] = 0.25f;
    return b;
  }
  double t[FB_MAX_TAPS], s = 0.0;
  for (int i = 0; i < b.n; ++i) {
    const double x = (double)(i - b.n / 2);
    t[i] = exp(-x * x / (2.0 * sigma * sigma));
    s += t[i];
  }
  for (int i = 0; i < b.n; ++i) b.t[i] = (float)(t[i] / s);
  return b;
}
inline PolyK poly_constants() {
  const int n = FB_POLY_N;
  const double sigma = 1.2;
  double g[2 * FB_POLY_N + 1], s = 0.0;
  for (int x = -n; x <= n; ++x) s += (g[x + n] = exp(-(double)(x * x) / (2.0 * sigma * sigma)));
  for (int i = 0; i <= 2 * n; ++i) g[i] /= s;
  // Gram matrix of (1, x, y, x^2, y^2, xy) under g(y) g(x): a = G00, b = G11, c = G33, d = G55
  double a = 0.0, b = 0.0, c = 0.0, d = 0.0;
  for (int y = -n; y <= n; ++y)
    for (int x = -n; x <= n; ++x) {
      const double gg = g[y + n] * g[x + n];
      a += gg;
      b += gg * x * x;
      c += gg * x * x * x * x;
      d += gg * x * x * y * y;
    }
  // inverse: rows 1, 2, 5 are diagonal; rows 0, 3, 4 form [[a b b] [b c d] [b d c]], det = (c - d)(a (c + d) - 2 b^2)
  const double q = a * (c + d) - 2.0 * b * b;
  PolyK p{};
  p.ig11 = (float)(1.0 / b);
  p.ig03 = (float)(-b / q);
  p.ig33 = (float)((a * c - b * b) / ((c - d) * q));
  p.ig55 = (float)(1.0 / d);
  for (int k = 0; k <= n; ++k) {
    p.g[k] = (float)g[n + k];
    p.xg[k] = (float)((double)k * g[n + k]);
    p.xxg[k] = (float)((double)(k * k) * g[n + k]);
  }
  return p;
}

// ---- device helpers ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int reflect101(int v, int n) {   // one reflection (radius < n), then a clamp for lanes
  v = v < 0 ? -v : v;                                        // whose result is never used
  v = v >= n ? 2 * n - 2 - v : v;
  return clampi(v, 0, n - 1);
}
// bilinear source taps of one axis: src = (dst + 0.5) (n_src / n_dst) - 0.5 in fp64, the fraction rounded once
__device__ __forceinline__ void resize_src(int dst, int n_dst, int n_src, int& i0, int& i1, float& f) {
  const double s = ((double)dst + 0.5) * ((double)n_src / (double)n_dst) - 0.5;
  const double fl = floor(s);
  f = (float)(s - fl);
  const int i = (int)fl;
  i0 = clampi(i, 0, n_src - 1);
  i1 = clampi(i + 1, 0, n_src - 1);
}

// ---- kernels ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fb_gray_kernel(const uint8_t* __restrict__ rgb, uint8_t* __restrict__ gray,
                                                      int fh, int fw, int h, int w) {
  const int f = blockIdx.z, y = blockIdx.y, x = blockIdx.x * 256 + threadIdx.x;
  if (x >= w) return;
  const uint8_t* p = rgb + (((size_t)f * fh + y) * fw + x) * 3;
  gray[((size_t)f * h + y) * w + x] = (uint8_t)((4899u * p[0] + 9617u * p[1] + 1868u * p[2] + 8192u) >> 14);
}

__global__ __launch_bounds__(256) void fb_hblur_kernel(const uint8_t* __restrict__ gray, float* __restrict__ out,
                                                       int h, int w, BlurTaps bt) {
  __shared__ float row[256 + FB_MAX_TAPS - 1];
  const int n = blockIdx.z, y = blockIdx.y, x0 = blockIdx.x * 256, r = bt.n / 2;
  const uint8_t* src = gray + ((size_t)n * h + y) * w;
  for (int i = threadIdx.x; i < 256 + 2 * r; i += 256) row[i] = (float)src[reflect101(x0 + i - r, w)];
  __syncthreads();
  const int x = x0 + threadIdx.x;
  if (x >= w) return;
  float acc = bt.t[0] * row[threadIdx.x];
  for (int i = 1; i < bt.n; ++i) acc = acc + bt.t[i] * row[threadIdx.x + i];
  out[((size_t)n * h + y) * w + x] = acc;
}

__global__ __launch_bounds__(256) void fb_vblur_resize_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                              int h, int w, int lh, int lw, BlurTaps bt) {
  const int n = blockIdx.z, xd = blockIdx.x * 64 + (threadIdx.x & 63), yd = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (xd >= lw || yd >= lh) return;
  int x0, x1, y0, y1;
  float fx, fy;
  resize_src(xd, lw, w, x0, x1, fx);
  resize_src(yd, lh, h, y0, y1, fy);
  const float* src = in + (size_t)n * h * w;
  const int r = bt.n / 2;
  float v00, v01, v10, v11;
  {
    int yy = reflect101(y0 - r, h);
    v00 = bt.t[0] * src[(size_t)yy * w + x0];
    v01 = bt.t[0] * src[(size_t)yy * w + x1];
    yy = reflect101(y1 - r, h);
    v10 = bt.t[0] * src[(size_t)yy * w + x0];
    v11 = bt.t[0] * src[(size_t)yy * w + x1];
  }
  for (int i = 1; i < bt.n; ++i) {
    const float t = bt.t[i];
    int yy = reflect101(y0 - r + i, h);
    v00 = v00 + t * src[(size_t)yy * w + x0];
    v01 = v01 + t * src[(size_t)yy * w + x1];
    yy = reflect101(y1 - r + i, h);
    v10 = v10 + t * src[(size_t)yy * w + x0];
    v11 = v11 + t * src[(size_t)yy * w + x1];
  }
  const float top = v00 * (1.0f - fx) + v01 * fx;
  const float bot = v10 * (1.0f - fx) + v11 * fx;
  out[((size_t)n * lh + yd) * lw + xd] = top * (1.0f - fy) + bot * fy;
}

__global__ __launch_bounds__(FB_THREADS) void fb_polyexp_kernel(const float* __restrict__ img, float* __restrict__ R,
                                                                int h, int w, PolyK pk) {
  __shared__ float in[FB_PE_IH * FB_PE_IW];
  __shared__ float v0[FB_TH * FB_PE_IW], v1[FB_TH * FB_PE_IW], v2[FB_TH * FB_PE_IW];
  const int tid = threadIdx.x, n = blockIdx.z;
  const int r0 = blockIdx.y * FB_TH, c0 = blockIdx.x * FB_TW;
  const float* src = img + (size_t)n * h * w;
  for (int i = tid; i < FB_PE_IH * FB_PE_IW; i += FB_THREADS) {       // replicate borders
    const int y = clampi(r0 + i / FB_PE_IW - FB_POLY_N, 0, h - 1), x = clampi(c0 + i % FB_PE_IW - FB_POLY_N, 0, w - 1);
    in[i] = src[(size_t)y * w + x];
  }
  __syncthreads();
  for (int i = tid; i < FB_TH * FB_PE_IW; i += FB_THREADS) {           // along y: g, x g, x^2 g
    const int r = i / FB_PE_IW + FB_POLY_N, c = i % FB_PE_IW;
    float s0 = pk.g[0] * in[r * FB_PE_IW + c], s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 1; k <= FB_POLY_N; ++k) {
      const float p = in[(r + k) * FB_PE_IW + c], q = in[(r - k) * FB_PE_IW + c];
      s0 = s0 + pk.g[k] * (p + q);
      s1 = k == 1 ? pk.xg[k] * (p - q) : s1 + pk.xg[k] * (p - q);
      s2 = k == 1 ? pk.xxg[k] * (p + q) : s2 + pk.xxg[k] * (p + q);
    }
    v0[i] = s0; v1[i] = s1; v2[i] = s2;
  }
  __syncthreads();
  const int c = tid % FB_TW;
  const size_t plane = (size_t)h * w;
  float* dst = R + (size_t)n * 5 * plane;
#pragma unroll
  for (int j = 0; j < FB_TH / (FB_THREADS / FB_TW); ++j) {
    const int r = (tid / FB_TW) * (FB_TH / (FB_THREADS / FB_TW)) + j;
    const int o = r * FB_PE_IW + c + FB_POLY_N;
    float b1 = pk.g[0] * v0[o], b3 = pk.g[0] * v1[o], b6 = pk.g[0] * v2[o], b2 = 0.f, b4 = 0.f, b5 = 0.f;
#pragma unroll
    for (int k = 1; k <= FB_POLY_N; ++k) {
      const float p0 = v0[o + k], q0 = v0[o - k], p1 = v1[o + k], q1 = v1[o - k], p2 = v2[o + k], q2 = v2[o - k];
      b1 = b1 + pk.g[k] * (p0 + q0);
      b2 = k == 1 ? pk.xg[k] * (p0 - q0) : b2 + pk.xg[k] * (p0 - q0);
      b4 = k == 1 ? pk.xxg[k] * (p0 + q0) : b4 + pk.xxg[k] * (p0 + q0);
      b3 = b3 + pk.g[k] * (p1 + q1);
      b5 = k == 1 ? pk.xg[k] * (p1 - q1) : b5 + pk.xg[k] * (p1 - q1);
      b6 = b6 + pk.g[k] * (p2 + q2);
    }
    const int y = r0 + r, x = c0 + c;
    if (y < h && x < w) {
      const size_t p = (size_t)y * w + x;
      dst[p] = b3 * pk.ig11;
      dst[plane + p] = b2 * pk.ig11;
      dst[2 * plane + p] = b1 * pk.ig03 + b6 * pk.ig33;
      dst[3 * plane + p] = b1 * pk.ig03 + b4 * pk.ig33;
      dst[4 * plane + p] = b5 * pk.ig55;
    }
  }
}

__device__ __forceinline__ float border_scale(int x, int y, int w, int h) {
  const float bd[5] = {0.14f, 0.14f, 0.4472f, 0.4472f, 0.4472f};
  float s = 1.0f;
#pragma unroll
  for (int d = 0; d < 5; ++d) s = x == d ? s * bd[d] : s;              // left, right, top, bottom: the order of the spec
#pragma unroll
  for (int d = 0; d < 5; ++d) s = x == w - 1 - d ? s * bd[d] : s;
#pragma unroll
  for (int d = 0; d < 5; ++d) s = y == d ? s * bd[d] : s;
#pragma unroll
  for (int d = 0; d < 5; ++d) s = y == h - 1 - d ? s * bd[d] : s;
  return s;
}

// R: (pairs + 1, 5, h, w); pair p takes images p and p + 1
__global__ __launch_bounds__(256) void fb_update_kernel(const float* __restrict__ R, const float* __restrict__ flow,
                                                        float* __restrict__ M, int h, int w) {
  const int n = blockIdx.z, x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= w || y >= h) return;
  const size_t plane = (size_t)h * w, p = (size_t)y * w + x;
  const float* R0 = R + (size_t)n * 5 * plane;
  const float* R1 = R0 + 5 * plane;
  const float2 d = ((const float2*)flow)[(size_t)n * plane + p];
  const float dx = d.x, dy = d.y;
  const float fx = (float)x + dx, fy = (float)y + dy;
  float r2, r3, r4, r5, r6;
  if (fx >= 0.f && fx < (float)(w - 1) && fy >= 0.f && fy < (float)(h - 1)) {   // 0 <= floor < n - 1; NaN: outside
    const float xf = floorf(fx), yf = floorf(fy);
    const int x1 = (int)xf, y1 = (int)yf;
    const float ax = fx - xf, ay = fy - yf;
    const float a00 = (1.0f - ax) * (1.0f - ay), a01 = ax * (1.0f - ay), a10 = (1.0f - ax) * ay, a11 = ax * ay;
    const float* q = R1 + (size_t)y1 * w + x1;
    float S[5];
#pragma unroll
    for (int c = 0; c < 5; ++c)
      S[c] = ((a00 * q[c * plane] + a01 * q[c * plane + 1]) + a10 * q[c * plane + w]) + a11 * q[c * plane + w + 1];
    r2 = (R0[p] - S[0]) * 0.5f;
    r3 = (R0[plane + p] - S[1]) * 0.5f;
    r4 = (R0[2 * plane + p] + S[2]) * 0.5f;
    r5 = (R0[3 * plane + p] + S[3]) * 0.5f;
    r6 = (R0[4 * plane + p] + S[4]) * 0.25f;
  } else {
    r2 = 0.f;
    r3 = 0.f;
    r4 = R0[2 * plane + p];
    r5 = R0[3 * plane + p];
    r6 = R0[4 * plane + p] * 0.5f;
  }
  r2 = r2 + (r4 * dy + r6 * dx);
  r3 = r3 + (r6 * dy + r5 * dx);
  const float s = border_scale(x, y, w, h);
  r2 = r2 * s; r3 = r3 * s; r4 = r4 * s; r5 = r5 * s; r6 = r6 * s;
  float* dst = M + (size_t)n * 5 * plane + p;
  dst[0] = r4 * r4 + r6 * r6;
  dst[plane] = (r4 + r5) * r6;
  dst[2 * plane] = r5 * r5 + r6 * r6;
  dst[3 * plane] = r4 * r2 + r6 * r3;
  dst[4 * plane] = r6 * r2 + r5 * r3;
}

__global__ __launch_bounds__(FB_THREADS) void fb_blur_solve_kernel(const float* __restrict__ M,
                                                                   float* __restrict__ flow, float* __restrict__ box,
                                                                   int h, int w) {
  __shared__ float xs[FB_BX_IH * FB_BX_IW];
  __shared__ float hs[FB_BX_IH * FB_TW];
  constexpr int RPT = FB_TH / (FB_THREADS / FB_TW);                     // rows per thread
  const int tid = threadIdx.x, n = blockIdx.z;
  const int r0 = blockIdx.y * FB_TH, c0 = blockIdx.x * FB_TW;
  const size_t plane = (size_t)h * w;
  const int c = tid % FB_TW, rb = (tid / FB_TW) * RPT;
  const float inv = (float)(1.0 / (FB_WIN * FB_WIN));
  float B[5][RPT];
#pragma unroll
  for (int ch = 0; ch < 5; ++ch) {
    const float* src = M + ((size_t)n * 5 + ch) * plane;
    if (ch) __syncthreads();
    for (int i = tid; i < FB_BX_IH * FB_BX_IW; i += FB_THREADS) {      // replicate borders
      const int y = clampi(r0 + i / FB_BX_IW - FB_WIN / 2, 0, h - 1), x = clampi(c0 + i % FB_BX_IW - FB_WIN / 2, 0, w - 1);
      xs[i] = src[(size_t)y * w + x];
    }
    __syncthreads();
    for (int i = tid; i < FB_BX_IH * FB_TW; i += FB_THREADS) {         // 15-sums along rows, left to right
      const int o = (i / FB_TW) * FB_BX_IW + i % FB_TW;
      float acc = xs[o];
#pragma unroll
      for (int k = 1; k < FB_WIN; ++k) acc = acc + xs[o + k];
      hs[i] = acc;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < RPT; ++j) {                                     // 15-sums along columns, top to bottom
      float acc = hs[(rb + j) * FB_TW + c];
#pragma unroll
      for (int k = 1; k < FB_WIN; ++k) acc = acc + hs[(rb + j + k) * FB_TW + c];
      B[ch][j] = acc * inv;
    }
  }
  const int x = c0 + c;
#pragma unroll
  for (int j = 0; j < RPT; ++j) {
    const int y = r0 + rb + j;
    if (y >= h || x >= w) continue;
    const size_t p = (size_t)y * w + x;
    const float g11 = B[0][j], g12 = B[1][j], g22 = B[2][j], h1 = B[3][j], h2 = B[4][j];
    if (box) {
#pragma unroll
      for (int ch = 0; ch < 5; ++ch) box[((size_t)n * 5 + ch) * plane + p] = B[ch][j];
    }
    const float idet = 1.0f / ((g11 * g22 - g12 * g12) + 1e-3f);
    float2 f;
    f.x = (g11 * h2 - g12 * h1) * idet;
    f.y = (g22 * h1 - g12 * h2) * idet;
    ((float2*)flow)[(size_t)n * plane + p] = f;
  }
}

__global__ __launch_bounds__(256) void fb_resize_flow_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                             int ih, int iw, int oh, int ow) {
  const int n = blockIdx.z, xd = blockIdx.x * 64 + (threadIdx.x & 63), yd = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (xd >= ow || yd >= oh) return;
  int x0, x1, y0, y1;
  float fx, fy;
  resize_src(xd, ow, iw, x0, x1, fx);
  resize_src(yd, oh, ih, y0, y1, fy);
  const float2* src = (const float2*)in + (size_t)n * ih * iw;
  const float2 a = src[(size_t)y0 * iw + x0], b = src[(size_t)y0 * iw + x1];
  const float2 c = src[(size_t)y1 * iw + x0], d = src[(size_t)y1 * iw + x1];
  const float gx = 1.0f - fx, gy = 1.0f - fy;
  float2 o;
  o.x = ((a.x * gx + b.x * fx) * gy + (c.x * gx + d.x * fx) * fy) * 2.0f;
  o.y = ((a.y * gx + b.y * fx) * gy + (c.y * gx + d.y * fx) * fy) * 2.0f;
  ((float2*)out)[((size_t)n * oh + yd) * ow + xd] = o;
}

__global__ __launch_bounds__(FB_EPE_THREADS) void flow_epe_kernel(const float* __restrict__ fa,
                                                                  const float* __restrict__ fb, int h, int w, int y0,
                                                                  int x0, int ch, int cw, double* __restrict__ mean) {
  __shared__ double red[FB_EPE_THREADS];
  const int n = blockIdx.x, tid = threadIdx.x;
  const float2* a = (const float2*)fa + (size_t)n * h * w;
  const float2* b = (const float2*)fb + (size_t)n * h * w;
  const long long cnt = (long long)ch * cw;
  double acc = 0.0;
  for (long long i = tid; i < cnt; i += FB_EPE_THREADS) {              // pixel i of the window -> thread i % 1024
    const int r = (int)(i / cw), c = (int)(i - (long long)r * cw);
    const size_t p = (size_t)(y0 + r) * w + (x0 + c);
    const float2 u = a[p], v = b[p];
    const float dx = u.x - v.x, dy = u.y - v.y;
    // the correctly rounded fp32 square root: fp64's 53 bits exceed 2 * 24 + 2, so rounding sqrt() of the fp32 sum
    // once more to fp32 is innocuous
    acc += (double)(float)sqrt((double)(dx * dx + dy * dy));
  }
  red[tid] = acc;
  __syncthreads();
  for (int s = FB_EPE_THREADS / 2; s > 0; s >>= 1) {                   // fixed tree
    if (tid < s) red[tid] = red[tid] + red[tid + s];
    __syncthreads();
  }
  if (tid == 0) mean[n] = red[0] / (double)cnt;
}

// ---- launches -----------------------------------------------------------------------------------------------------
inline bool size_ok(int n, int h, int w) {
  return n > 0 && n <= 65535 && h >= 16 && w >= 16 && h <= 32768 && w <= 32768;
}
inline dim3 pix_grid(int h, int w, int n) { return dim3(cdiv(w, 64), cdiv(h, 4), n); }
inline dim3 tile_grid(int h, int w, int n) { return dim3(cdiv(w, FB_TW), cdiv(h, FB_TH), n); }

int launch_gray(const uint8_t* rgb, int frames, int fh, int fw, int h, int w, uint8_t* gray, hipStream_t st) {
  hipLaunchKernelGGL(fb_gray_kernel, dim3(cdiv(w, 256), h, frames), dim3(256), 0, st, rgb, gray, fh, fw, h, w);
  return check_launch("fb_gray");
}
int launch_level_image(const uint8_t* gray, int n, int h, int w, int level, float* tmp, float* out, hipStream_t st) {
  const BlurTaps bt = blur_taps(level);
  const int lh = level_dim(h, level), lw = level_dim(w, level);
  hipLaunchKernelGGL(fb_hblur_kernel, dim3(cdiv(w, 256), h, n), dim3(256), 0, st, gray, tmp, h, w, bt);
  int rc = check_launch("fb_hblur");
  if (rc != TG_OK) return rc;
  hipLaunchKernelGGL(fb_vblur_resize_kernel, pix_grid(lh, lw, n), dim3(256), 0, st, (const float*)tmp, out, h, w, lh,
                     lw, bt);
  return check_launch("fb_vblur_resize");
}
int launch_polyexp(const float* img, int n, int h, int w, float* R, hipStream_t st) {
  static const PolyK pk = poly_constants();
  hipLaunchKernelGGL(fb_polyexp_kernel, tile_grid(h, w, n), dim3(FB_THREADS), 0, st, img, R, h, w, pk);
  return check_launch("fb_polyexp");
}
int launch_update(const float* R, const float* flow, float* M, int pairs, int h, int w, hipStream_t st) {
  hipLaunchKernelGGL(fb_update_kernel, pix_grid(h, w, pairs), dim3(256), 0, st, R, flow, M, h, w);
  return check_launch("fb_update");
}
int launch_blur_solve(const float* M, float* flow, float* box, int pairs, int h, int w, hipStream_t st) {
  hipLaunchKernelGGL(fb_blur_solve_kernel, tile_grid(h, w, pairs), dim3(FB_THREADS), 0, st, M, flow, box, h, w);
  return check_launch("fb_blur_solve");
}
int launch_resize_flow(const float* in, int ih, int iw, float* out, int oh, int ow, int pairs, hipStream_t st) {
  hipLaunchKernelGGL(fb_resize_flow_kernel, pix_grid(oh, ow, pairs), dim3(256), 0, st, in, out, ih, iw, oh, ow);
  return check_launch("fb_resize_flow");
}

// workspace of the composite: offsets in bytes, each a multiple of 256
struct FbLayout {
  size_t gray, tmp, img, R, M, flow1, total;
};
inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
inline FbLayout fb_layout(int pairs, int h, int w) {
  const size_t frames = (size_t)pairs + 1, hw = (size_t)h * w;
  const size_t hw1 = (size_t)level_dim(h, 1) * level_dim(w, 1);        // odd levels' flows live in the workspace
  FbLayout l;
  size_t o = 0;
  l.gray = o;  o += up256(frames * hw);
  l.tmp = o;   o += up256(frames * hw * 4);
  l.img = o;   o += up256(frames * hw * 4);
  l.R = o;     o += up256(frames * 5 * hw * 4);
  l.M = o;     o += up256((size_t)pairs * 5 * hw * 4);
  l.flow1 = o; o += up256((size_t)pairs * hw1 * 8);
  l.total = o;
  return l;
}

}  // namespace
}  // namespace tg

using namespace tg;

extern "C" int tg_fb_level_size(int h, int w, int level, int* level_h, int* level_w) {
  TG_REQUIRE(size_ok(1, h, w) && level >= 0 && level <= FB_MAX_LEVEL && level_h && level_w, TG_E_ARG,
             "fb_level_size: %dx%d level %d (16 <= h, w <= 32768, level 0..3)", h, w, level);
  *level_h = level_dim(h, level);
  *level_w = level_dim(w, level);
  return top_level(h, w);
}

extern "C" int tg_fb_gray_u8(const uint8_t* rgb_hwc, int frames, int frame_h, int frame_w, int h, int w,
                             uint8_t* gray, tg_stream_t stream) {
  TG_REQUIRE(rgb_hwc && gray, TG_E_ARG, "fb_gray_u8: null pointer");
  TG_REQUIRE(size_ok(frames, h, w) && frame_h >= h && frame_w >= w && frame_h <= 32768 && frame_w <= 32768, TG_E_ARG,
             "fb_gray_u8: frames=%d of %dx%d, region %dx%d (at least 16x16, inside the frame)", frames, frame_h,
             frame_w, h, w);
  return launch_gray(rgb_hwc, frames, frame_h, frame_w, h, w, gray, (hipStream_t)stream);
}

extern "C" int tg_fb_level_image(const uint8_t* gray, int n, int h, int w, int level, float* tmp, float* out,
                                 tg_stream_t stream) {
  TG_REQUIRE(gray && tmp && out, TG_E_ARG, "fb_level_image: null pointer");
  TG_REQUIRE(size_ok(n, h, w) && level >= 0 && level <= top_level(h, w), TG_E_ARG,
             "fb_level_image: n=%d %dx%d level %d (levels 0..%d)", n, h, w, level, size_ok(1, h, w) ? top_level(h, w) : 0);
  return launch_level_image(gray, n, h, w, level, tmp, out, (hipStream_t)stream);
}

extern "C" int tg_fb_polyexp(const float* img, int n, int h, int w, float* r_out, tg_stream_t stream) {
  TG_REQUIRE(img && r_out, TG_E_ARG, "fb_polyexp: null pointer");
  TG_REQUIRE(size_ok(n, h, w), TG_E_ARG, "fb_polyexp: n=%d %dx%d (at least 16x16)", n, h, w);
  return launch_polyexp(img, n, h, w, r_out, (hipStream_t)stream);
}

extern "C" int tg_fb_update_matrices(const float* r, const float* flow, float* m_out, int pairs, int h, int w,
                                     tg_stream_t stream) {
  TG_REQUIRE(r && flow && m_out, TG_E_ARG, "fb_update_matrices: null pointer");
  TG_REQUIRE(size_ok(pairs, h, w) && pairs < 65535, TG_E_ARG, "fb_update_matrices: pairs=%d %dx%d", pairs, h, w);
  return launch_update(r, flow, m_out, pairs, h, w, (hipStream_t)stream);
}

extern "C" int tg_fb_blur_solve(const float* m, float* flow_out, float* box_out, int pairs, int h, int w,
                                tg_stream_t stream) {
  TG_REQUIRE(m && flow_out, TG_E_ARG, "fb_blur_solve: null pointer");
  TG_REQUIRE(size_ok(pairs, h, w), TG_E_ARG, "fb_blur_solve: pairs=%d %dx%d", pairs, h, w);
  return launch_blur_solve(m, flow_out, box_out, pairs, h, w, (hipStream_t)stream);
}

extern "C" int tg_fb_resize_flow(const float* flow_in, int h_in, int w_in, float* flow_out, int h_out, int w_out,
                                 int pairs, tg_stream_t stream) {
  TG_REQUIRE(flow_in && flow_out, TG_E_ARG, "fb_resize_flow: null pointer");
  TG_REQUIRE(size_ok(pairs, h_in, w_in) && size_ok(pairs, h_out, w_out), TG_E_ARG,
             "fb_resize_flow: pairs=%d %dx%d -> %dx%d", pairs, h_in, w_in, h_out, w_out);
  return launch_resize_flow(flow_in, h_in, w_in, flow_out, h_out, w_out, pairs, (hipStream_t)stream);
}

extern "C" int64_t tg_farneback_workspace_bytes(int pairs, int h, int w) {
  if (!size_ok(pairs, h, w) || pairs >= 65535) return -1;
  return (int64_t)fb_layout(pairs, h, w).total;
}

extern "C" int tg_farneback_flow_u8(const uint8_t* rgb_hwc, int frames, int frame_h, int frame_w, int h, int w,
                                    float* flow_out, void* workspace, size_t workspace_bytes, tg_stream_t stream) {
  TG_REQUIRE(rgb_hwc && flow_out && workspace, TG_E_ARG, "farneback_flow_u8: null pointer");
  TG_REQUIRE(frames >= 2 && size_ok(frames, h, w) && frame_h >= h && frame_w >= w && frame_h <= 32768 &&
                 frame_w <= 32768, TG_E_ARG,
             "farneback_flow_u8: frames=%d of %dx%d, region %dx%d (two frames, at least 16x16, inside the frame)",
             frames, frame_h, frame_w, h, w);
  const int pairs = frames - 1;
  const FbLayout l = fb_layout(pairs, h, w);
  TG_REQUIRE(workspace_bytes >= l.total, TG_E_ARG, "farneback_flow_u8: workspace of %zu bytes, %zu needed",
             workspace_bytes, l.total);
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  uint8_t* gray = (uint8_t*)(ws + l.gray);
  float *tmp = (float*)(ws + l.tmp), *img = (float*)(ws + l.img), *R = (float*)(ws + l.R), *M = (float*)(ws + l.M);
  float* flow1 = (float*)(ws + l.flow1);
  int rc = launch_gray(rgb_hwc, frames, frame_h, frame_w, h, w, gray, st);
  if (rc != TG_OK) return rc;
  const int top = top_level(h, w);
  float* prev = nullptr;
  int ph = 0, pw = 0;
  for (int k = top; k >= 0; --k) {
    const int lh = level_dim(h, k), lw = level_dim(w, k);
    float* flow = (k & 1) ? flow1 : flow_out;                            // level 0 is the result; level 2 fits into it
    if ((rc = launch_level_image(gray, frames, h, w, k, tmp, img, st)) != TG_OK) return rc;
    if ((rc = launch_polyexp(img, frames, lh, lw, R, st)) != TG_OK) return rc;
    if (prev) {
      if ((rc = launch_resize_flow(prev, ph, pw, flow, lh, lw, pairs, st)) != TG_OK) return rc;
    } else {
      if (hipMemsetAsync(flow, 0, (size_t)pairs * lh * lw * 8, st) != hipSuccess) return check_launch("fb_zero_flow");
    }
    if ((rc = launch_update(R, flow, M, pairs, lh, lw, st)) != TG_OK) return rc;
    for (int it = 0; it < FB_ITERS; ++it) {
      if ((rc = launch_blur_solve(M, flow, nullptr, pairs, lh, lw, st)) != TG_OK) return rc;
      if (it < FB_ITERS - 1 && (rc = launch_update(R, flow, M, pairs, lh, lw, st)) != TG_OK) return rc;
    }
    prev = flow; ph = lh; pw = lw;
  }
  return TG_OK;
}

extern "C" int tg_flow_epe_mean(const float* flow_a, const float* flow_b, int n, int h, int w, int y0, int x0, int ch,
                                int cw, double* mean_f64, tg_stream_t stream) {
  TG_REQUIRE(flow_a && flow_b && mean_f64, TG_E_ARG, "flow_epe_mean: null pointer");
  TG_REQUIRE(n > 0 && n <= 1 << 20 && h > 0 && w > 0 && h <= 32768 && w <= 32768 && y0 >= 0 && x0 >= 0 && ch > 0 &&
                 cw > 0 && y0 <= h - ch && x0 <= w - cw, TG_E_ARG,
             "flow_epe_mean: n=%d flows of %dx%d, window (%d,%d) %dx%d does not lie inside", n, h, w, y0, x0, ch, cw);
  hipLaunchKernelGGL(flow_epe_kernel, dim3(n), dim3(FB_EPE_THREADS), 0, (hipStream_t)stream, flow_a, flow_b, h, w, y0,
                     x0, ch, cw, mean_f64);
  return check_launch("flow_epe_mean");
}
