// Planar YUV 4:2:0 (I420, 8 bit) in and out of the stream: what a decoder hands over and an
// encoder takes, converted on the device so that 1.5 bytes per pixel cross PCIe instead of 3.
//
//   tg_yuv420_to_rgb_f32: I420 -> fp32 CHW RGB in [0,1] (the LR slot of infer_stream).  Chroma is up-sampled
//     bilinearly in exact integers (sixteenths), then ONE fp32 matrix step, then the clamp: no uint8 RGB in between.
//   tg_rgb_u8_to_yuv420:  uint8 HWC RGB (what the HR tail writes) -> I420 in exact 16.16 integer arithmetic: the
//     specification is the integer formula itself, tests/yuv_ref.py restates it in numpy and the bytes must be equal.
//
// Both are pure streaming kernels.  A thread owns whole chroma samples: a 2-row x 4-pixel strip on the way out (two U
// and two V samples, 24 bytes read, 12 written), one row x 4 pixels on the way in (12 floats written).  The wide
// accesses (dwords of RGB / Y, 16-bit chroma pairs, float4 rows) are taken only where every address is provably
// aligned -- width a multiple of 4 and aligned base pointers, which makes the row stride 3W, the plane offsets and
// the frame stride multiples of 4 as well; every other shape (W = 2 mod 4: rows 2-byte aligned; odd sizes: odd plane
// offsets) takes the byte-wide form of the same kernel.
#include "tg_common.h"

namespace tg {

struct yuv_q {          // rint(M * 65536) of the RGB -> YCbCr matrix, rows Y / Cb / Cr, and the luma offset
  int y[3], cb[3], cr[3], yo;
};

struct yuv_f {          // the inverse step on integers: R = ky*(Y-yo) + rv*dv ... with du, dv = C16 - 2048 (sixteenths)
  float ky, rv, gu, gv, bu;
  int yo;
};

// {bt601, bt709} x {limited, full}; the four tables of DESIGN.md section 7e (tests/test_yuv_cpu.py recomputes them
// from Kr and Kb in fp64)
static const yuv_q Q_TABLE[2][2] = {
    {{{16829, 33039, 6416}, {-9714, -19071, 28784}, {28784, -24103, -4681}, 16},
     {{19595, 38470, 7471}, {-11058, -21710, 32768}, {32768, -27439, -5329}, 0}},
    {{{11966, 40254, 4064}, {-6596, -22189, 28784}, {28784, -26145, -2639}, 16},
     {{13933, 46871, 4732}, {-7509, -25259, 32768}, {32768, -29763, -3005}, 0}}};

static yuv_f inverse_coefficients(int matrix, int full_range) {
  const double kr = matrix == TG_YUV_BT601 ? 0.299 : 0.2126, kb = matrix == TG_YUV_BT601 ? 0.114 : 0.0722;
  const double kg = 1.0 - kr - kb;
  const double ys = full_range ? 255.0 : 219.0, cs16 = 16.0 * (full_range ? 255.0 : 224.0);
  yuv_f f;
  f.ky = (float)(1.0 / ys);
  f.rv = (float)(2.0 * (1.0 - kr) / cs16);
  f.bu = (float)(2.0 * (1.0 - kb) / cs16);
  f.gu = (float)(-(2.0 * kb * (1.0 - kb) / kg) / cs16);
  f.gv = (float)(-(2.0 * kr * (1.0 - kr) / kg) / cs16);
  f.yo = full_range ? 0 : 16;
  return f;
}

// clip(acc >> sh, 0, 255) of a floor shift, written as a clamp of the accumulator followed by a logical shift (the
// same value: a negative acc gives 0, one of 256 << sh or more gives 255).  With the clamp AFTER the shift hipcc fuses
// two neighbours into one v_ashr_pk_u8_i32, whose 16-bit result it then packed into the Y dword as if the upper half
// of the register were zero: bytes 2 and 3 of the store came out wrong on the MI355X.
__device__ __forceinline__ int shift_clip_u8(int acc, int sh) {
  const int top = (256 << sh) - 1;
  acc = acc < 0 ? 0 : (acc > top ? top : acc);
  return (int)((unsigned)acc >> sh);
}
__device__ __forceinline__ int dot3(const int q[3], const int p[3]) { return q[0] * p[0] + q[1] * p[1] + q[2] * p[2]; }
__device__ __forceinline__ float clamp01(float v) { return __builtin_fminf(__builtin_fmaxf(v, 0.f), 1.f); }

// ---- RGB uint8 HWC -> I420 ---------------------------------------------------------------------------------------
// thread = rows 2j, 2j+1 x pixels 4*tx .. 4*tx+3 of frame k.  H and W are even, so a strip holds 2 or 4 pixels.
template <bool VEC, bool LEFT>
__global__ __launch_bounds__(256) void rgb_u8_to_yuv420_kernel(const uint8_t* __restrict__ rgb,
                                                               uint8_t* __restrict__ yuv, int H, int W, int strips,
                                                               long long total, yuv_q q) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int tx = (int)(i % strips);
  const long long r = i / strips;
  const int j = (int)(r % (H >> 1));
  const long long k = r / (H >> 1);
  const int x0 = 4 * tx, cw = W >> 1, ch = H >> 1;
  const int npx = W - x0 < 4 ? W - x0 : 4;                        // 2 or 4
  const long long row3 = 3LL * W;
  const uint8_t* src = rgb + (k * H + 2 * j) * row3 + 3 * x0;
  int p[2][4][3];
#pragma unroll
  for (int rr = 0; rr < 2; ++rr) {
    if (VEC) {                                                    // 12 bytes at a 4-byte aligned address
      const uint32_t* s4 = reinterpret_cast<const uint32_t*>(src + rr * row3);
      const uint32_t a = s4[0], b = s4[1], c = s4[2];
      const uint32_t by[12] = {a & 255, (a >> 8) & 255, (a >> 16) & 255, a >> 24, b & 255, (b >> 8) & 255,
                               (b >> 16) & 255, b >> 24, c & 255, (c >> 8) & 255, (c >> 16) & 255, c >> 24};
#pragma unroll
      for (int e = 0; e < 12; ++e) p[rr][e / 3][e % 3] = (int)by[e];
    } else {
#pragma unroll
      for (int e = 0; e < 12; ++e) p[rr][e / 3][e % 3] = e < 3 * npx ? (int)src[rr * row3 + e] : 0;
    }
  }
  uint8_t* yp = yuv + k * ((long long)H * W + 2LL * ch * cw);
  uint8_t* up = yp + (long long)H * W;
  uint8_t* vp = up + (long long)ch * cw;
  const int yround = (q.yo << 16) + (1 << 15);
#pragma unroll
  for (int rr = 0; rr < 2; ++rr) {
    int yv[4];
#pragma unroll
    for (int x = 0; x < 4; ++x) yv[x] = shift_clip_u8(dot3(q.y, p[rr][x]) + yround, 16);
    uint8_t* dst = yp + (long long)(2 * j + rr) * W + x0;
    if (VEC) {
      *reinterpret_cast<uint32_t*>(dst) =
          (uint32_t)yv[0] | ((uint32_t)yv[1] << 8) | ((uint32_t)yv[2] << 16) | ((uint32_t)yv[3] << 24);
    } else {
#pragma unroll
      for (int x = 0; x < 4; ++x)
        if (x < npx) dst[x] = (uint8_t)yv[x];
    }
  }
  int uo[2], vo[2];
#pragma unroll
  for (int c2 = 0; c2 < 2; ++c2) {
    int s[3];
    if (LEFT) {                                                   // (1, 2, 1) over x-1, x, x+1 at x = 2i, x-1 clamped to 0
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        int acc = 0;
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
          int left;
          if (c2 == 1) left = p[rr][1][c];
          else left = x0 == 0 ? p[rr][0][c] : (int)src[rr * row3 - 3 + c];      // the left neighbour's last column
          acc += left + 2 * p[rr][2 * c2][c] + p[rr][2 * c2 + 1][c];
        }
        s[c] = acc;
      }
      uo[c2] = shift_clip_u8(dot3(q.cb, s) + (128 << 19) + (1 << 18), 19);
      vo[c2] = shift_clip_u8(dot3(q.cr, s) + (128 << 19) + (1 << 18), 19);
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c)
        s[c] = p[0][2 * c2][c] + p[0][2 * c2 + 1][c] + p[1][2 * c2][c] + p[1][2 * c2 + 1][c];
      uo[c2] = shift_clip_u8(dot3(q.cb, s) + (128 << 18) + (1 << 17), 18);
      vo[c2] = shift_clip_u8(dot3(q.cr, s) + (128 << 18) + (1 << 17), 18);
    }
  }
  const long long co = (long long)j * cw + 2 * tx;
  if (VEC) {                                                      // cw and both plane offsets are even here
    *reinterpret_cast<uint16_t*>(up + co) = (uint16_t)(uo[0] | (uo[1] << 8));
    *reinterpret_cast<uint16_t*>(vp + co) = (uint16_t)(vo[0] | (vo[1] << 8));
  } else {
    up[co] = (uint8_t)uo[0];
    vp[co] = (uint8_t)vo[0];
    if (npx == 4) {
      up[co + 1] = (uint8_t)uo[1];
      vp[co + 1] = (uint8_t)vo[1];
    }
  }
}

// ---- I420 -> fp32 CHW RGB ----------------------------------------------------------------------------------------
// thread = row y x pixels 4*tx .. 4*tx+3 of frame k.  The strip needs chroma columns 2*tx-1 .. 2*tx+2 of two chroma
// rows, every index clamped into the plane (so the loads are in bounds for the pixels past an odd width too).
template <bool VEC, bool LEFT>
__global__ __launch_bounds__(256) void yuv420_to_rgb_f32_kernel(const uint8_t* __restrict__ yuv,
                                                                float* __restrict__ rgb, int h, int w, int strips,
                                                                long long total, yuv_f f) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int tx = (int)(i % strips);
  const long long r = i / strips;
  const int y = (int)(r % h);
  const long long k = r / h;
  const int x0 = 4 * tx, ch = (h + 1) >> 1, cw = (w + 1) >> 1;
  const uint8_t* yp = yuv + k * ((long long)h * w + 2LL * ch * cw);
  const uint8_t* up = yp + (long long)h * w;
  const uint8_t* vp = up + (long long)ch * cw;
  // rows: even y -> (y/2 - 1, y/2) x (1, 3); odd y -> ((y-1)/2, (y+1)/2) x (3, 1)
  int r0 = (y & 1) ? (y - 1) >> 1 : (y >> 1) - 1, r1 = r0 + 1;
  const int w0 = (y & 1) ? 3 : 1, w1 = 4 - w0;
  r0 = r0 < 0 ? 0 : r0;
  r1 = r1 > ch - 1 ? ch - 1 : r1;
  int u[4], v[4];                                                 // vertical sums of columns 2*tx-1 .. 2*tx+2, in quarters
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    int c = 2 * tx - 1 + m;
    c = c < 0 ? 0 : (c > cw - 1 ? cw - 1 : c);
    u[m] = w0 * (int)up[(long long)r0 * cw + c] + w1 * (int)up[(long long)r1 * cw + c];
    v[m] = w0 * (int)vp[(long long)r0 * cw + c] + w1 * (int)vp[(long long)r1 * cw + c];
  }
  int u16[4], v16[4];                                             // sixteenths
  if (LEFT) {                                                     // even x: its own column; odd x: the two around it
    u16[0] = 4 * u[1]; u16[1] = 2 * (u[1] + u[2]); u16[2] = 4 * u[2]; u16[3] = 2 * (u[2] + u[3]);
    v16[0] = 4 * v[1]; v16[1] = 2 * (v[1] + v[2]); v16[2] = 4 * v[2]; v16[3] = 2 * (v[2] + v[3]);
  } else {                                                        // the row rule again
    u16[0] = u[0] + 3 * u[1]; u16[1] = 3 * u[1] + u[2]; u16[2] = u[1] + 3 * u[2]; u16[3] = 3 * u[2] + u[3];
    v16[0] = v[0] + 3 * v[1]; v16[1] = 3 * v[1] + v[2]; v16[2] = v[1] + 3 * v[2]; v16[3] = 3 * v[2] + v[3];
  }
  int yy[4];
  const uint8_t* ysrc = yp + (long long)y * w + x0;
  if (VEC) {
    const uint32_t a = *reinterpret_cast<const uint32_t*>(ysrc);
    yy[0] = (int)(a & 255); yy[1] = (int)((a >> 8) & 255); yy[2] = (int)((a >> 16) & 255); yy[3] = (int)(a >> 24);
  } else {
#pragma unroll
    for (int x = 0; x < 4; ++x) yy[x] = x0 + x < w ? (int)ysrc[x] : 0;
  }
  float R[4], G[4], B[4];
#pragma unroll
  for (int x = 0; x < 4; ++x) {
    const float yf = f.ky * (float)(yy[x] - f.yo);
    const float du = (float)(u16[x] - 2048), dv = (float)(v16[x] - 2048);
    R[x] = clamp01(__builtin_fmaf(f.rv, dv, yf));
    G[x] = clamp01(__builtin_fmaf(f.gv, dv, __builtin_fmaf(f.gu, du, yf)));
    B[x] = clamp01(__builtin_fmaf(f.bu, du, yf));
  }
  const long long plane = (long long)h * w;
  float* dst = rgb + k * 3 * plane + (long long)y * w + x0;
  if (VEC) {
    *reinterpret_cast<f32x4*>(dst) = f32x4{R[0], R[1], R[2], R[3]};
    *reinterpret_cast<f32x4*>(dst + plane) = f32x4{G[0], G[1], G[2], G[3]};
    *reinterpret_cast<f32x4*>(dst + 2 * plane) = f32x4{B[0], B[1], B[2], B[3]};
  } else {
#pragma unroll
    for (int x = 0; x < 4; ++x)
      if (x0 + x < w) {
        dst[x] = R[x];
        dst[plane + x] = G[x];
        dst[2 * plane + x] = B[x];
      }
  }
}

static bool yuv_enums_ok(int matrix, int full_range, int siting) {
  return (matrix == TG_YUV_BT601 || matrix == TG_YUV_BT709) && (full_range == 0 || full_range == 1) &&
         (siting == TG_YUV_CENTER || siting == TG_YUV_LEFT);
}

// ---- 10 and 12 bits per sample ---------------------------------------------------------------
// A sample is a 16-bit little-endian word with d significant bits; the frame layout is I420's with 2-byte samples.
//   tg_rgb_f32_to_yuv420p16: the fp32 CHW HR state -> I420 at d bits.  ONE float step per value (clamp, times 65535,
//     round half even) gives 16-bit integers q; everything behind it is exact 64-bit integer arithmetic on Q =
//     rint(M_d * 2^24), and tests/yuv_depth_ref.py restates it in numpy: the words must be equal.
//   tg_yuv420p16_to_rgb_f32: the 8-bit input kernel again on 16-bit samples (one above 2^d - 1 is read as 2^d - 1).
// The thread-to-pixel map is the 8-bit kernels': 2 rows x 4 pixels on the way out (six float4 loads, two 8-byte Y stores,
// two 4-byte chroma stores), one row x 4 pixels on the way in (one 8-byte Y load, three float4 stores); neighbouring
// lanes touch neighbouring 16 / 8 / 4 bytes of every plane.  The wide forms are taken only where every address is
// aligned (width a multiple of 4, fp32 base 16-byte and sample base 8-byte aligned: all row, plane and frame strides
// follow); every other shape or placement takes the element-wide form, whose sample stores are 2 bytes wide.
struct yuv_q24 {        // rint(M_d * 2^24), rows Y / Cb / Cr; luma offset, chroma mid value and top code at depth d
  int y[3], cb[3], cr[3], yo, mid, top;
};

// [depth 10, 12][bt601, bt709][limited, full]: the tables of DESIGN.md section 7k (tests/test_yuv_depth_cpu.py
// recomputes them from Kr and Kb in fp64)
static const yuv_q24 Q24_TABLE[2][2][2] = {
    {{{{67054, 131640, 25566}, {-38705, -75985, 114690}, {114690, -96038, -18651}, 64, 512, 1023},
      {{78306, 153731, 29856}, {-44191, -86755, 130946}, {130946, -109651, -21295}, 0, 512, 1023}},
     {{{47678, 160390, 16192}, {-26280, -88409, 114690}, {114690, -104173, -10516}, 64, 512, 1023},
      {{55678, 187305, 18909}, {-30006, -100940, 130946}, {130946, -118939, -12007}, 0, 512, 1023}}},
    {{{{268214, 526561, 102262}, {-154818, -303941, 458759}, {458759, -384153, -74606}, 256, 2048, 4095},
      {{313452, 615373, 119510}, {-176892, -347276, 524168}, {524168, -438925, -85243}, 0, 2048, 4095}},
     {{{190710, 641561, 64766}, {-105122, -353637, 458759}, {458759, -416693, -42066}, 256, 2048, 4095},
      {{222876, 749770, 75690}, {-120110, -404058, 524168}, {524168, -476105, -48063}, 0, 2048, 4095}}}};

static yuv_f inverse_coefficients_deep(int matrix, int full_range, int depth) {
  const double kr = matrix == TG_YUV_BT601 ? 0.299 : 0.2126, kb = matrix == TG_YUV_BT601 ? 0.114 : 0.0722;
  const double kg = 1.0 - kr - kb;
  const double top = (double)((1 << depth) - 1), up = (double)(1 << (depth - 8));
  const double ys = full_range ? top : 219.0 * up, cs16 = 16.0 * (full_range ? top : 224.0 * up);
  yuv_f f;
  f.ky = (float)(1.0 / ys);
  f.rv = (float)(2.0 * (1.0 - kr) / cs16);
  f.bu = (float)(2.0 * (1.0 - kb) / cs16);
  f.gu = (float)(-(2.0 * kb * (1.0 - kb) / kg) / cs16);
  f.gv = (float)(-(2.0 * kr * (1.0 - kr) / kg) / cs16);
  f.yo = full_range ? 0 : 16 << (depth - 8);
  return f;
}

// the one float step of the output direction: v < 0 and NaN give 0 (both comparisons are false for a NaN, so the first
// one decides), v > 1 gives 65535; one fp32 multiply, one round half even
__device__ __forceinline__ int quantize16(float v) {
  v = v > 0.f ? v : 0.f;
  v = v < 1.f ? v : 1.f;
  return (int)__builtin_rintf(v * 65535.0f);
}
// clip(acc >> sh, 0, top) of a floor shift on 64 bits, as shift_clip_u8 writes it: the clamp comes first, the shift is
// logical, and no packed 16-bit shift can be formed from it (section 7e's compiler note)
__device__ __forceinline__ unsigned shift_clip_top(long long acc, int sh, int top) {
  const long long lim = ((long long)(top + 1) << sh) - 1;
  acc = acc < 0 ? 0 : (acc > lim ? lim : acc);
  return (unsigned)((unsigned long long)acc >> sh);
}
__device__ __forceinline__ long long dot3_64(const int q[3], const int p[3]) {
  return (long long)q[0] * p[0] + (long long)q[1] * p[1] + (long long)q[2] * p[2];
}

// thread = rows 2j, 2j+1 x pixels 4*tx .. 4*tx+3 of frame k.  H and W are even, so a strip holds 2 or 4 pixels.
template <bool VEC, bool LEFT>
__global__ __launch_bounds__(256) void rgb_f32_to_yuv420p16_kernel(const float* __restrict__ rgb,
                                                                   uint16_t* __restrict__ yuv, int H, int W, int strips,
                                                                   long long total, yuv_q24 q) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int tx = (int)(i % strips);
  const long long r = i / strips;
  const int j = (int)(r % (H >> 1));
  const long long k = r / (H >> 1);
  const int x0 = 4 * tx, cw = W >> 1, ch = H >> 1;
  const int npx = W - x0 < 4 ? W - x0 : 4;                        // 2 or 4
  const long long plane = (long long)H * W;
  const float* src = rgb + k * 3 * plane + (long long)(2 * j) * W + x0;
  int p[2][4][3];
#pragma unroll
  for (int rr = 0; rr < 2; ++rr)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float* s = src + c * plane + (long long)rr * W;
      if (VEC) {                                                  // 16 bytes at a 16-byte aligned address
        const f32x4 v = *reinterpret_cast<const f32x4*>(s);
        p[rr][0][c] = quantize16(v.x); p[rr][1][c] = quantize16(v.y);
        p[rr][2][c] = quantize16(v.z); p[rr][3][c] = quantize16(v.w);
      } else {
#pragma unroll
        for (int x = 0; x < 4; ++x) p[rr][x][c] = x < npx ? quantize16(s[x]) : 0;
      }
    }
  uint16_t* yp = yuv + k * (plane + 2LL * ch * cw);
  uint16_t* up = yp + plane;
  uint16_t* vp = up + (long long)ch * cw;
  const long long yround = ((long long)q.yo << 24) + (1LL << 23);
#pragma unroll
  for (int rr = 0; rr < 2; ++rr) {
    unsigned yv[4];
#pragma unroll
    for (int x = 0; x < 4; ++x) yv[x] = shift_clip_top(dot3_64(q.y, p[rr][x]) + yround, 24, q.top);
    uint16_t* dst = yp + (long long)(2 * j + rr) * W + x0;
    if (VEC) {
      *reinterpret_cast<u32x2*>(dst) = u32x2{yv[0] | (yv[1] << 16), yv[2] | (yv[3] << 16)};
    } else {
#pragma unroll
      for (int x = 0; x < 4; ++x)
        if (x < npx) dst[x] = (uint16_t)yv[x];
    }
  }
  unsigned uo[2], vo[2];
#pragma unroll
  for (int c2 = 0; c2 < 2; ++c2) {
    int s[3];
    if (LEFT) {                                                   // (1, 2, 1) over x-1, x, x+1 at x = 2i, x-1 clamped to 0
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        int acc = 0;
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
          int left;
          if (c2 == 1) left = p[rr][1][c];
          else left = x0 == 0 ? p[rr][0][c] : quantize16(src[c * plane + (long long)rr * W - 1]);   // the strip before
          acc += left + 2 * p[rr][2 * c2][c] + p[rr][2 * c2 + 1][c];
        }
        s[c] = acc;
      }
      const long long cround = ((long long)q.mid << 27) + (1LL << 26);
      uo[c2] = shift_clip_top(dot3_64(q.cb, s) + cround, 27, q.top);
      vo[c2] = shift_clip_top(dot3_64(q.cr, s) + cround, 27, q.top);
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c)
        s[c] = p[0][2 * c2][c] + p[0][2 * c2 + 1][c] + p[1][2 * c2][c] + p[1][2 * c2 + 1][c];
      const long long cround = ((long long)q.mid << 26) + (1LL << 25);
      uo[c2] = shift_clip_top(dot3_64(q.cb, s) + cround, 26, q.top);
      vo[c2] = shift_clip_top(dot3_64(q.cr, s) + cround, 26, q.top);
    }
  }
  const long long co = (long long)j * cw + 2 * tx;
  if (VEC) {                                                      // cw and both plane offsets are even here
    *reinterpret_cast<uint32_t*>(up + co) = uo[0] | (uo[1] << 16);
    *reinterpret_cast<uint32_t*>(vp + co) = vo[0] | (vo[1] << 16);
  } else {
    up[co] = (uint16_t)uo[0];
    vp[co] = (uint16_t)vo[0];
    if (npx == 4) {
      up[co + 1] = (uint16_t)uo[1];
      vp[co + 1] = (uint16_t)vo[1];
    }
  }
}

// thread = row y x pixels 4*tx .. 4*tx+3 of frame k, as yuv420_to_rgb_f32_kernel; `top` = 2^d - 1 bounds every sample,
// `mid16` = 16 * 2^(d-1) is the chroma mid value in sixteenths
template <bool VEC, bool LEFT>
__global__ __launch_bounds__(256) void yuv420p16_to_rgb_f32_kernel(const uint16_t* __restrict__ yuv,
                                                                   float* __restrict__ rgb, int h, int w, int strips,
                                                                   long long total, yuv_f f, int top, int mid16) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int tx = (int)(i % strips);
  const long long r = i / strips;
  const int y = (int)(r % h);
  const long long k = r / h;
  const int x0 = 4 * tx, ch = (h + 1) >> 1, cw = (w + 1) >> 1;
  const uint16_t* yp = yuv + k * ((long long)h * w + 2LL * ch * cw);
  const uint16_t* up = yp + (long long)h * w;
  const uint16_t* vp = up + (long long)ch * cw;
  int r0 = (y & 1) ? (y - 1) >> 1 : (y >> 1) - 1, r1 = r0 + 1;
  const int w0 = (y & 1) ? 3 : 1, w1 = 4 - w0;
  r0 = r0 < 0 ? 0 : r0;
  r1 = r1 > ch - 1 ? ch - 1 : r1;
  auto sample = [top](const uint16_t* p, long long at) { const int s = (int)p[at]; return s > top ? top : s; };
  int u[4], v[4];                                                 // vertical sums of columns 2*tx-1 .. 2*tx+2, in quarters
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    int c = 2 * tx - 1 + m;
    c = c < 0 ? 0 : (c > cw - 1 ? cw - 1 : c);
    u[m] = w0 * sample(up, (long long)r0 * cw + c) + w1 * sample(up, (long long)r1 * cw + c);
    v[m] = w0 * sample(vp, (long long)r0 * cw + c) + w1 * sample(vp, (long long)r1 * cw + c);
  }
  int u16[4], v16[4];                                             // sixteenths
  if (LEFT) {
    u16[0] = 4 * u[1]; u16[1] = 2 * (u[1] + u[2]); u16[2] = 4 * u[2]; u16[3] = 2 * (u[2] + u[3]);
    v16[0] = 4 * v[1]; v16[1] = 2 * (v[1] + v[2]); v16[2] = 4 * v[2]; v16[3] = 2 * (v[2] + v[3]);
  } else {
    u16[0] = u[0] + 3 * u[1]; u16[1] = 3 * u[1] + u[2]; u16[2] = u[1] + 3 * u[2]; u16[3] = 3 * u[2] + u[3];
    v16[0] = v[0] + 3 * v[1]; v16[1] = 3 * v[1] + v[2]; v16[2] = v[1] + 3 * v[2]; v16[3] = 3 * v[2] + v[3];
  }
  int yy[4];
  const uint16_t* ysrc = yp + (long long)y * w + x0;
  if (VEC) {                                                      // 8 bytes at an 8-byte aligned address
    const u32x2 a = *reinterpret_cast<const u32x2*>(ysrc);
    yy[0] = (int)(a.x & 65535u); yy[1] = (int)(a.x >> 16); yy[2] = (int)(a.y & 65535u); yy[3] = (int)(a.y >> 16);
  } else {
#pragma unroll
    for (int x = 0; x < 4; ++x) yy[x] = x0 + x < w ? (int)ysrc[x] : 0;
  }
  float R[4], G[4], B[4];
#pragma unroll
  for (int x = 0; x < 4; ++x) {
    const int ys = yy[x] > top ? top : yy[x];
    const float yf = f.ky * (float)(ys - f.yo);
    const float du = (float)(u16[x] - mid16), dv = (float)(v16[x] - mid16);
    R[x] = clamp01(__builtin_fmaf(f.rv, dv, yf));
    G[x] = clamp01(__builtin_fmaf(f.gv, dv, __builtin_fmaf(f.gu, du, yf)));
    B[x] = clamp01(__builtin_fmaf(f.bu, du, yf));
  }
  const long long plane = (long long)h * w;
  float* dst = rgb + k * 3 * plane + (long long)y * w + x0;
  if (VEC) {
    *reinterpret_cast<f32x4*>(dst) = f32x4{R[0], R[1], R[2], R[3]};
    *reinterpret_cast<f32x4*>(dst + plane) = f32x4{G[0], G[1], G[2], G[3]};
    *reinterpret_cast<f32x4*>(dst + 2 * plane) = f32x4{B[0], B[1], B[2], B[3]};
  } else {
#pragma unroll
    for (int x = 0; x < 4; ++x)
      if (x0 + x < w) {
        dst[x] = R[x];
        dst[plane + x] = G[x];
        dst[2 * plane + x] = B[x];
      }
  }
}

// ---- 4:2:0, 4:2:2 and 4:4:4 at 8, 10 and 12 bits, any (Kr, Kb) -------------------------------
// One kernel template per direction over (sample type T, SX, SY, VEC, LEFT): T = uint8_t is the 8-bit arithmetic of
// section 7e (32-bit accumulators, shift 16, uint8 HWC RGB on the way out), T = uint16_t the one of section 7k (64-bit
// accumulators, shift 24, fp32 CHW RGB); (SX, SY) is the chroma sub-sampling, (2,2) | (2,1) | (1,1).  The arithmetic is
// the four kernels' above with a sub-sampled axis switched on or off, through the same helpers, so (2,2) gives their
// floats, bytes and words.  The integer tables are computed on the host from (Kr, Kb) and passed as a kernel argument.
//
// Thread map: one row x 4 pixels on the way in; SY rows x 4 pixels on the way out, so that a thread owns whole chroma
// samples (4 / SX per plane).
//
// Alignment of the wide form (VEC), taken only when W % 4 == 0 and the bases are aligned as the entry points above
// test (samples: 4 bytes at 8 bit, 8 bytes at 16 bit; fp32: 16 bytes; uint8 RGB: 4 bytes).  In samples, with W = 4 m:
//   row stride W, and a strip's x0 = 4 tx: multiples of 4.  Y plane H W: a multiple of 4.
//   chroma plane ch cw -- 4:2:0 (on the way in ch = ceil(H/2)): ch 2m, even, and two planes ch W, a multiple of 4;
//   4:2:2: H 2m, even, two planes H W; 4:4:4: H W, a multiple of 4 already.
//   So every frame starts a multiple of 4 samples behind the base, U starts a multiple of 4 behind the frame, and V an
//   even number of samples (a multiple of 4 at 4:4:4) behind U.  A strip's chroma run starts at j cw + x0 / SX: even
//   for SX = 2 (cw = 2m, a run of 2 samples), a multiple of 4 for SX = 1 (cw = 4m, a run of 4).
//   Hence: Y runs of 4 samples and 4:4:4 chroma runs of 4 are aligned to 4 samples (a dword at 8 bit, 8 bytes at 16
//   bit), chroma runs of 2 to 2 samples (a 16-bit word / a dword).  fp32 CHW: plane H W and row W are multiples of 4
//   floats, so every float4 is 16-byte aligned; uint8 HWC: row 3W = 12m and 3 x0 = 12 tx, so the three dwords are.
// Every other shape or placement takes the element-wide form of the same kernel.
struct yuv_qp {         // rint(M * 2^16) (8 bit) or rint(M_d * 2^24), rows Y / Cb / Cr; luma offset, chroma mid, top code
  int y[3], cb[3], cr[3], yo, mid, top;
};

static bool yuv_kr_kb(int matrix, double* kr, double* kb) {
  switch (matrix) {
    case TG_YUV_BT601: *kr = 0.299; *kb = 0.114; return true;
    case TG_YUV_BT709: *kr = 0.2126; *kb = 0.0722; return true;
    case TG_YUV_BT2020: *kr = 0.2627; *kb = 0.0593; return true;      // non-constant luminance
  }
  return false;
}

// yo, ys, cs, mid at `depth` bits (8: section 7e's, above: section 7k's)
static void yuv_scales(int depth, int full_range, int* yo, double* ys, double* cs, int* mid) {
  const int up = depth - 8;
  const double top = (double)((1 << depth) - 1);
  *yo = full_range ? 0 : 16 << up;
  *ys = full_range ? top : (double)(219 << up);
  *cs = full_range ? top : (double)(224 << up);
  *mid = 128 << up;
}

// Q in fp64, rounded half even (the default rounding mode): from RGB levels 0..255 times 2^16 at depth 8, from 16-bit
// codes 0..65535 times 2^24 above.  For BT601 / BT709 these are Q_TABLE / Q24_TABLE entry for entry.
static yuv_qp forward_table(int matrix, int full_range, int depth) {
  double kr = 0, kb = 0, ys, cs;
  yuv_qp q;
  yuv_kr_kb(matrix, &kr, &kb);
  yuv_scales(depth, full_range, &q.yo, &ys, &cs, &q.mid);
  q.top = (1 << depth) - 1;
  const double kg = 1.0 - kr - kb;
  const double in = depth == 8 ? 255.0 : 65535.0, one = depth == 8 ? 65536.0 : 16777216.0;
  const double m[3][3] = {{kr * ys / in, kg * ys / in, kb * ys / in},
                          {-kr / (2 * (1 - kb)) * cs / in, -kg / (2 * (1 - kb)) * cs / in, 0.5 * cs / in},
                          {0.5 * cs / in, -kg / (2 * (1 - kr)) * cs / in, -kb / (2 * (1 - kr)) * cs / in}};
  for (int c = 0; c < 3; ++c) {
    q.y[c] = (int)__builtin_rint(m[0][c] * one);
    q.cb[c] = (int)__builtin_rint(m[1][c] * one);
    q.cr[c] = (int)__builtin_rint(m[2][c] * one);
  }
  return q;
}

static yuv_f inverse_table(int matrix, int full_range, int depth) {       // inverse_coefficients(_deep) for any (Kr, Kb)
  double kr = 0, kb = 0, ys, cs;
  int mid;
  yuv_f f;
  yuv_kr_kb(matrix, &kr, &kb);
  yuv_scales(depth, full_range, &f.yo, &ys, &cs, &mid);
  const double kg = 1.0 - kr - kb, cs16 = 16.0 * cs;
  f.ky = (float)(1.0 / ys);
  f.rv = (float)(2.0 * (1.0 - kr) / cs16);
  f.bu = (float)(2.0 * (1.0 - kb) / cs16);
  f.gu = (float)(-(2.0 * kb * (1.0 - kb) / kg) / cs16);
  f.gv = (float)(-(2.0 * kr * (1.0 - kr) / kg) / cs16);
  return f;
}

// what differs between the two sample types on the way out: the RGB source, the accumulator and the base shift
template <typename T> struct yuv_out;
template <> struct yuv_out<uint8_t> {
  typedef uint8_t src_t;
  typedef int acc_t;
  static constexpr int BASE = 16;
  static __device__ __forceinline__ acc_t dot(const int q[3], const int p[3]) { return dot3(q, p); }
  static __device__ __forceinline__ unsigned clip(acc_t acc, int sh, int) { return (unsigned)shift_clip_u8(acc, sh); }
  // pixels x0 .. x0+3 of row `row` of frame k (HWC bytes); the ones from npx on are 0
  template <bool VEC>
  static __device__ __forceinline__ void load(const src_t* rgb, long long k, int H, int W, int row, int x0, int npx,
                                              int p[4][3]) {
    const uint8_t* s = rgb + (k * H + row) * (3LL * W) + 3 * x0;
    if (VEC) {                                                    // 12 bytes at a 4-byte aligned address
      const uint32_t* s4 = reinterpret_cast<const uint32_t*>(s);
      const uint32_t a = s4[0], b = s4[1], c = s4[2];
      const uint32_t by[12] = {a & 255, (a >> 8) & 255, (a >> 16) & 255, a >> 24, b & 255, (b >> 8) & 255,
                               (b >> 16) & 255, b >> 24, c & 255, (c >> 8) & 255, (c >> 16) & 255, c >> 24};
#pragma unroll
      for (int e = 0; e < 12; ++e) p[e / 3][e % 3] = (int)by[e];
    } else {
#pragma unroll
      for (int e = 0; e < 12; ++e) p[e / 3][e % 3] = e < 3 * npx ? (int)s[e] : 0;
    }
  }
  // pixel x0 - 1 of that row (x0 >= 4): the strip before's last column
  static __device__ __forceinline__ void left(const src_t* rgb, long long k, int H, int W, int row, int x0, int l[3]) {
    const uint8_t* s = rgb + (k * H + row) * (3LL * W) + 3 * x0 - 3;
    l[0] = (int)s[0]; l[1] = (int)s[1]; l[2] = (int)s[2];
  }
};
template <> struct yuv_out<uint16_t> {
  typedef float src_t;
  typedef long long acc_t;
  static constexpr int BASE = 24;
  static __device__ __forceinline__ acc_t dot(const int q[3], const int p[3]) { return dot3_64(q, p); }
  static __device__ __forceinline__ unsigned clip(acc_t acc, int sh, int top) { return shift_clip_top(acc, sh, top); }
  template <bool VEC>
  static __device__ __forceinline__ void load(const src_t* rgb, long long k, int H, int W, int row, int x0, int npx,
                                              int p[4][3]) {
    const long long plane = (long long)H * W;
    const float* s = rgb + k * 3 * plane + (long long)row * W + x0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (VEC) {                                                  // 16 bytes at a 16-byte aligned address
        const f32x4 v = *reinterpret_cast<const f32x4*>(s + c * plane);
        p[0][c] = quantize16(v.x); p[1][c] = quantize16(v.y); p[2][c] = quantize16(v.z); p[3][c] = quantize16(v.w);
      } else {
#pragma unroll
        for (int x = 0; x < 4; ++x) p[x][c] = x < npx ? quantize16(s[c * plane + x]) : 0;
      }
    }
  }
  static __device__ __forceinline__ void left(const src_t* rgb, long long k, int H, int W, int row, int x0, int l[3]) {
    const long long plane = (long long)H * W;
    const float* s = rgb + k * 3 * plane + (long long)row * W + x0 - 1;
    l[0] = quantize16(s[0]); l[1] = quantize16(s[plane]); l[2] = quantize16(s[2 * plane]);
  }
};

// N = 4 | 2 samples to dst; the wide form is one store of N samples (dst aligned to N samples), the other one writes
// the first cnt of them one by one
template <bool VEC, int N>
__device__ __forceinline__ void store_samples(uint8_t* dst, const unsigned v[N], int cnt) {
  if (VEC) {
    if (N == 4) *reinterpret_cast<uint32_t*>(dst) = v[0] | (v[1] << 8) | (v[2 % N] << 16) | (v[3 % N] << 24);
    else *reinterpret_cast<uint16_t*>(dst) = (uint16_t)(v[0] | (v[1] << 8));
  } else {
#pragma unroll
    for (int x = 0; x < N; ++x)
      if (x < cnt) dst[x] = (uint8_t)v[x];
  }
}
template <bool VEC, int N>
__device__ __forceinline__ void store_samples(uint16_t* dst, const unsigned v[N], int cnt) {
  if (VEC) {
    if (N == 4) *reinterpret_cast<u32x2*>(dst) = u32x2{v[0] | (v[1] << 16), v[2 % N] | (v[3 % N] << 16)};
    else *reinterpret_cast<uint32_t*>(dst) = v[0] | (v[1] << 16);
  } else {
#pragma unroll
    for (int x = 0; x < N; ++x)
      if (x < cnt) dst[x] = (uint16_t)v[x];
  }
}

// thread = rows SY*j .. SY*j + SY-1 x pixels 4*tx .. 4*tx+3 of frame k.  H is a multiple of SY and W one of SX (the
// entry points test it), so a strip holds whole chroma samples: npx is 2 or 4 for SX = 2, 1 .. 4 for SX = 1.
template <typename T, int SX, int SY, bool VEC, bool LEFT>
__global__ __launch_bounds__(256) void rgb_to_yuv_planar_kernel(const typename yuv_out<T>::src_t* __restrict__ rgb,
                                                                T* __restrict__ yuv, int H, int W, int strips,
                                                                long long total, yuv_qp q) {
  typedef yuv_out<T> O;
  typedef typename O::acc_t acc_t;
  static_assert((SX == 2 || SX == 1) && (SY == 2 || SY == 1) && SY <= SX, "4:2:0, 4:2:2 or 4:4:4");
  static_assert(SX == 2 || !LEFT, "the siting matters along a sub-sampled axis only");
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int tx = (int)(i % strips);
  const long long r = i / strips;
  const int ch = H / SY, cw = W / SX;
  const int j = (int)(r % ch);
  const long long k = r / ch;
  const int x0 = 4 * tx;
  const int npx = W - x0 < 4 ? W - x0 : 4;
  const long long plane = (long long)H * W, cplane = (long long)ch * cw;
  int p[SY][4][3];
#pragma unroll
  for (int rr = 0; rr < SY; ++rr) O::template load<VEC>(rgb, k, H, W, SY * j + rr, x0, npx, p[rr]);
  T* yp = yuv + k * (plane + 2 * cplane);
  T* up = yp + plane;
  T* vp = up + cplane;
  const acc_t yround = ((acc_t)q.yo << O::BASE) + ((acc_t)1 << (O::BASE - 1));
#pragma unroll
  for (int rr = 0; rr < SY; ++rr) {
    unsigned yv[4];
#pragma unroll
    for (int x = 0; x < 4; ++x) yv[x] = O::clip(O::dot(q.y, p[rr][x]) + yround, O::BASE, q.top);
    store_samples<VEC, 4>(yp + (long long)(SY * j + rr) * W + x0, yv, npx);
  }
  constexpr int NC = 4 / SX;                                      // chroma samples of the strip, per plane
  constexpr int T2 = (SX == 2 ? (LEFT ? 2 : 1) : 0) + (SY - 1);   // log2 of the total tap weight
  constexpr int SH = O::BASE + T2;
  const acc_t cround = ((acc_t)q.mid << SH) + ((acc_t)1 << (SH - 1));
  unsigned uo[NC], vo[NC];
#pragma unroll
  for (int c2 = 0; c2 < NC; ++c2) {
    int s[3] = {0, 0, 0};
#pragma unroll
    for (int rr = 0; rr < SY; ++rr) {
      if (SX == 1) {                                              // the pixel itself
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] += p[rr][c2][c];
      } else if (LEFT) {                                          // (1, 2, 1) over x-1, x, x+1 at x = 2i, x-1 clamped to 0
        int l[3] = {p[rr][(2 * c2 + 3) % 4][0], p[rr][(2 * c2 + 3) % 4][1], p[rr][(2 * c2 + 3) % 4][2]};
        if (c2 == 0) {
          if (x0 == 0) { l[0] = p[rr][0][0]; l[1] = p[rr][0][1]; l[2] = p[rr][0][2]; }
          else O::left(rgb, k, H, W, SY * j + rr, x0, l);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] += l[c] + 2 * p[rr][(2 * c2) % 4][c] + p[rr][(2 * c2 + 1) % 4][c];
      } else {                                                    // the pair
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] += p[rr][(2 * c2) % 4][c] + p[rr][(2 * c2 + 1) % 4][c];
      }
    }
    uo[c2] = O::clip(O::dot(q.cb, s) + cround, SH, q.top);
    vo[c2] = O::clip(O::dot(q.cr, s) + cround, SH, q.top);
  }
  const long long co = (long long)j * cw + NC * tx;
  const int ncs = npx / SX;                                       // chroma samples inside the frame
  store_samples<VEC, NC>(up + co, uo, ncs);
  store_samples<VEC, NC>(vp + co, vo, ncs);
}

// thread = row y x pixels 4*tx .. 4*tx+3 of frame k, as yuv420_to_rgb_f32_kernel.  `top` = 2^d - 1 bounds every 16-bit
// sample, `mid16` = 16 * mid.  Along a sub-sampled axis the taps are the ones above; along one that is not, the sample
// of the pixel itself times 4.  Every chroma index is clamped into the plane, so the loads of the pixels past the
// width are in bounds too.
template <typename T, int SX, int SY, bool VEC, bool LEFT>
__global__ __launch_bounds__(256) void yuv_planar_to_rgb_f32_kernel(const T* __restrict__ yuv, float* __restrict__ rgb,
                                                                    int h, int w, int strips, long long total, yuv_f f,
                                                                    int top, int mid16) {
  static_assert((SX == 2 || SX == 1) && (SY == 2 || SY == 1) && SY <= SX, "4:2:0, 4:2:2 or 4:4:4");
  static_assert(SX == 2 || !LEFT, "the siting matters along a sub-sampled axis only");
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int tx = (int)(i % strips);
  const long long r = i / strips;
  const int y = (int)(r % h);
  const long long k = r / h;
  const int x0 = 4 * tx, ch = (h + SY - 1) / SY, cw = (w + SX - 1) / SX;
  const T* yp = yuv + k * ((long long)h * w + 2LL * ch * cw);
  const T* up = yp + (long long)h * w;
  const T* vp = up + (long long)ch * cw;
  auto sample = [top](const T* p, long long at) {
    const int s = (int)p[at];
    return sizeof(T) == 1 ? s : (s > top ? top : s);
  };
  int r0, r1, w0, w1;                                             // two chroma rows and their weights, in quarters
  if (SY == 2) {                                                  // even y -> (y/2 - 1, y/2) x (1, 3); odd y -> (3, 1)
    r0 = (y & 1) ? (y - 1) >> 1 : (y >> 1) - 1;
    r1 = r0 + 1;
    w0 = (y & 1) ? 3 : 1;
    w1 = 4 - w0;
    r0 = r0 < 0 ? 0 : r0;
    r1 = r1 > ch - 1 ? ch - 1 : r1;
  } else {
    r0 = r1 = y;
    w0 = 4;
    w1 = 0;
  }
  int u[4], v[4];                                                 // vertical sums in quarters: columns 2*tx-1 .. 2*tx+2, or x0 .. x0+3
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    int c = SX == 2 ? 2 * tx - 1 + m : x0 + m;
    c = c < 0 ? 0 : (c > cw - 1 ? cw - 1 : c);
    if (SY == 2) {
      u[m] = w0 * sample(up, (long long)r0 * cw + c) + w1 * sample(up, (long long)r1 * cw + c);
      v[m] = w0 * sample(vp, (long long)r0 * cw + c) + w1 * sample(vp, (long long)r1 * cw + c);
    } else {
      u[m] = 4 * sample(up, (long long)r0 * cw + c);
      v[m] = 4 * sample(vp, (long long)r0 * cw + c);
    }
  }
  int u16[4], v16[4];                                             // sixteenths
  if (SX == 1) {
#pragma unroll
    for (int x = 0; x < 4; ++x) { u16[x] = 4 * u[x]; v16[x] = 4 * v[x]; }
  } else if (LEFT) {                                              // even x: its own column; odd x: the two around it
    u16[0] = 4 * u[1]; u16[1] = 2 * (u[1] + u[2]); u16[2] = 4 * u[2]; u16[3] = 2 * (u[2] + u[3]);
    v16[0] = 4 * v[1]; v16[1] = 2 * (v[1] + v[2]); v16[2] = 4 * v[2]; v16[3] = 2 * (v[2] + v[3]);
  } else {                                                        // the row rule again
    u16[0] = u[0] + 3 * u[1]; u16[1] = 3 * u[1] + u[2]; u16[2] = u[1] + 3 * u[2]; u16[3] = 3 * u[2] + u[3];
    v16[0] = v[0] + 3 * v[1]; v16[1] = 3 * v[1] + v[2]; v16[2] = v[1] + 3 * v[2]; v16[3] = 3 * v[2] + v[3];
  }
  int yy[4];
  const T* ysrc = yp + (long long)y * w + x0;
  if (VEC && sizeof(T) == 1) {                                    // 4 bytes at a 4-byte aligned address
    const uint32_t a = *reinterpret_cast<const uint32_t*>(ysrc);
    yy[0] = (int)(a & 255); yy[1] = (int)((a >> 8) & 255); yy[2] = (int)((a >> 16) & 255); yy[3] = (int)(a >> 24);
  } else if (VEC) {                                               // 8 bytes at an 8-byte aligned address
    const u32x2 a = *reinterpret_cast<const u32x2*>(ysrc);
    yy[0] = (int)(a.x & 65535u); yy[1] = (int)(a.x >> 16); yy[2] = (int)(a.y & 65535u); yy[3] = (int)(a.y >> 16);
  } else {
#pragma unroll
    for (int x = 0; x < 4; ++x) yy[x] = x0 + x < w ? (int)ysrc[x] : 0;
  }
  float R[4], G[4], B[4];
#pragma unroll
  for (int x = 0; x < 4; ++x) {
    const int ys = sizeof(T) == 1 ? yy[x] : (yy[x] > top ? top : yy[x]);
    const float yf = f.ky * (float)(ys - f.yo);
    const float du = (float)(u16[x] - mid16), dv = (float)(v16[x] - mid16);
    R[x] = clamp01(__builtin_fmaf(f.rv, dv, yf));
    G[x] = clamp01(__builtin_fmaf(f.gv, dv, __builtin_fmaf(f.gu, du, yf)));
    B[x] = clamp01(__builtin_fmaf(f.bu, du, yf));
  }
  const long long plane = (long long)h * w;
  float* dst = rgb + k * 3 * plane + (long long)y * w + x0;
  if (VEC) {
    *reinterpret_cast<f32x4*>(dst) = f32x4{R[0], R[1], R[2], R[3]};
    *reinterpret_cast<f32x4*>(dst + plane) = f32x4{G[0], G[1], G[2], G[3]};
    *reinterpret_cast<f32x4*>(dst + 2 * plane) = f32x4{B[0], B[1], B[2], B[3]};
  } else {
#pragma unroll
    for (int x = 0; x < 4; ++x)
      if (x0 + x < w) {
        dst[x] = R[x];
        dst[plane + x] = G[x];
        dst[2 * plane + x] = B[x];
      }
  }
}

static bool yuv_planar_enums_ok(int chroma, int matrix, int full_range, int siting) {
  return (chroma == TG_YUV_420 || chroma == TG_YUV_422 || chroma == TG_YUV_444) &&
         (matrix == TG_YUV_BT601 || matrix == TG_YUV_BT709 || matrix == TG_YUV_BT2020) &&
         (full_range == 0 || full_range == 1) && (siting == TG_YUV_CENTER || siting == TG_YUV_LEFT);
}

template <typename T, int SX, int SY>
static void launch_planar_out(bool vec, bool left, dim3 grid, hipStream_t st, const typename yuv_out<T>::src_t* rgb,
                              T* yuv, int H, int W, int strips, long long total, const yuv_qp& q) {
  constexpr bool L = SX == 2;                                     // (4:4:4 has the one form: the siting is not looked at)
  const dim3 block(256);
  if (vec) {
    if (left) hipLaunchKernelGGL((rgb_to_yuv_planar_kernel<T, SX, SY, true, L>), grid, block, 0, st, rgb, yuv, H, W, strips, total, q);
    else hipLaunchKernelGGL((rgb_to_yuv_planar_kernel<T, SX, SY, true, false>), grid, block, 0, st, rgb, yuv, H, W, strips, total, q);
  } else {
    if (left) hipLaunchKernelGGL((rgb_to_yuv_planar_kernel<T, SX, SY, false, L>), grid, block, 0, st, rgb, yuv, H, W, strips, total, q);
    else hipLaunchKernelGGL((rgb_to_yuv_planar_kernel<T, SX, SY, false, false>), grid, block, 0, st, rgb, yuv, H, W, strips, total, q);
  }
}

template <typename T, int SX, int SY>
static void launch_planar_in(bool vec, bool left, dim3 grid, hipStream_t st, const T* yuv, float* rgb, int h, int w,
                             int strips, long long total, const yuv_f& f, int top, int mid16) {
  constexpr bool L = SX == 2;
  const dim3 block(256);
  if (vec) {
    if (left) hipLaunchKernelGGL((yuv_planar_to_rgb_f32_kernel<T, SX, SY, true, L>), grid, block, 0, st, yuv, rgb, h, w, strips, total, f, top, mid16);
    else hipLaunchKernelGGL((yuv_planar_to_rgb_f32_kernel<T, SX, SY, true, false>), grid, block, 0, st, yuv, rgb, h, w, strips, total, f, top, mid16);
  } else {
    if (left) hipLaunchKernelGGL((yuv_planar_to_rgb_f32_kernel<T, SX, SY, false, L>), grid, block, 0, st, yuv, rgb, h, w, strips, total, f, top, mid16);
    else hipLaunchKernelGGL((yuv_planar_to_rgb_f32_kernel<T, SX, SY, false, false>), grid, block, 0, st, yuv, rgb, h, w, strips, total, f, top, mid16);
  }
}

// the checks and the launch of the output direction for one sample type; `base_ok` = the wide form's base alignments
template <typename T>
static int rgb_to_yuv_planar(const char* name, const typename yuv_out<T>::src_t* rgb, T* yuv, int n, int H, int W,
                             int chroma, int depth, int matrix, int full_range, int siting, bool base_ok,
                             tg_stream_t stream) {
  TG_REQUIRE(yuv_planar_enums_ok(chroma, matrix, full_range, siting), TG_E_ARG,
             "%s: chroma=%d matrix=%d full_range=%d siting=%d", name, chroma, matrix, full_range, siting);
  const int sx = chroma == TG_YUV_444 ? 1 : 2, sy = chroma == TG_YUV_420 ? 2 : 1;
  TG_REQUIRE(n >= 1 && H >= sy && W >= sx && H % sy == 0 && W % sx == 0, TG_E_ARG,
             "%s: n=%d H=%d W=%d (n >= 1; 4:2:0: H and W even, 4:2:2: W even)", name, n, H, W);
  const int strips = (W + 3) / 4;
  const long long total = (long long)n * (H / sy) * strips;
  TG_REQUIRE(total < (1LL << 38), TG_E_SHAPE, "%s: %lld strips", name, total);
  const bool vec = W % 4 == 0 && base_ok, left = siting == TG_YUV_LEFT && sx == 2;
  const yuv_qp q = forward_table(matrix, full_range, depth);
  const dim3 grid((unsigned)((total + 255) / 256));
  const hipStream_t st = (hipStream_t)stream;
  if (chroma == TG_YUV_420) launch_planar_out<T, 2, 2>(vec, left, grid, st, rgb, yuv, H, W, strips, total, q);
  else if (chroma == TG_YUV_422) launch_planar_out<T, 2, 1>(vec, left, grid, st, rgb, yuv, H, W, strips, total, q);
  else launch_planar_out<T, 1, 1>(vec, left, grid, st, rgb, yuv, H, W, strips, total, q);
  return check_launch(name);
}

template <typename T>
static int yuv_planar_to_rgb(const T* yuv, float* rgb, int n, int h, int w, int chroma, int depth, int matrix,
                             int full_range, int siting, bool base_ok, tg_stream_t stream) {
  const int sx = chroma == TG_YUV_444 ? 1 : 2;
  const int strips = (w + 3) / 4;
  const long long total = (long long)n * h * strips;
  TG_REQUIRE(total < (1LL << 38), TG_E_SHAPE, "yuv_planar_to_rgb_f32: %lld strips", total);
  const bool vec = w % 4 == 0 && base_ok, left = siting == TG_YUV_LEFT && sx == 2;
  const yuv_f f = inverse_table(matrix, full_range, depth);
  const int top = (1 << depth) - 1, mid16 = 16 << (depth - 1);
  const dim3 grid((unsigned)((total + 255) / 256));
  const hipStream_t st = (hipStream_t)stream;
  if (chroma == TG_YUV_420) launch_planar_in<T, 2, 2>(vec, left, grid, st, yuv, rgb, h, w, strips, total, f, top, mid16);
  else if (chroma == TG_YUV_422) launch_planar_in<T, 2, 1>(vec, left, grid, st, yuv, rgb, h, w, strips, total, f, top, mid16);
  else launch_planar_in<T, 1, 1>(vec, left, grid, st, yuv, rgb, h, w, strips, total, f, top, mid16);
  return check_launch("yuv_planar_to_rgb_f32");
}

}  // namespace tg

extern "C" int tg_yuv_planar_to_rgb_f32(const void* yuv, float* rgb_chw, int n, int h, int w, int chroma, int depth,
                                        int matrix, int full_range, int siting, tg_stream_t stream) {
  TG_REQUIRE(yuv && rgb_chw, TG_E_ARG, "yuv_planar_to_rgb_f32: null pointer");
  TG_REQUIRE(depth == 8 || depth == 10 || depth == 12, TG_E_ARG, "yuv_planar_to_rgb_f32: depth=%d (8, 10 or 12)", depth);
  TG_REQUIRE((depth == 8 || (uintptr_t)yuv % 2 == 0) && (uintptr_t)rgb_chw % 4 == 0, TG_E_ARG,
             "yuv_planar_to_rgb_f32: 16-bit samples are 2-byte aligned and rgb_chw 4-byte aligned");
  TG_REQUIRE(n >= 1 && h >= 2 && w >= 2, TG_E_ARG, "yuv_planar_to_rgb_f32: n=%d h=%d w=%d (n >= 1, h, w >= 2)", n, h, w);
  TG_REQUIRE(tg::yuv_planar_enums_ok(chroma, matrix, full_range, siting), TG_E_ARG,
             "yuv_planar_to_rgb_f32: chroma=%d matrix=%d full_range=%d siting=%d", chroma, matrix, full_range, siting);
  const bool f16 = (uintptr_t)rgb_chw % 16 == 0;
  if (depth == 8)
    return tg::yuv_planar_to_rgb<uint8_t>((const uint8_t*)yuv, rgb_chw, n, h, w, chroma, depth, matrix, full_range,
                                          siting, f16 && (uintptr_t)yuv % 4 == 0, stream);
  return tg::yuv_planar_to_rgb<uint16_t>((const uint16_t*)yuv, rgb_chw, n, h, w, chroma, depth, matrix, full_range,
                                         siting, f16 && (uintptr_t)yuv % 8 == 0, stream);
}

extern "C" int tg_rgb_u8_to_yuv_planar(const uint8_t* rgb_hwc, uint8_t* yuv, int n, int H, int W, int chroma,
                                       int matrix, int full_range, int siting, tg_stream_t stream) {
  TG_REQUIRE(rgb_hwc && yuv, TG_E_ARG, "rgb_u8_to_yuv_planar: null pointer");
  return tg::rgb_to_yuv_planar<uint8_t>("rgb_u8_to_yuv_planar", rgb_hwc, yuv, n, H, W, chroma, 8, matrix, full_range,
                                        siting, (uintptr_t)rgb_hwc % 4 == 0 && (uintptr_t)yuv % 4 == 0, stream);
}

extern "C" int tg_rgb_f32_to_yuv_planar16(const float* rgb_chw, uint16_t* yuv, int n, int H, int W, int chroma,
                                          int depth, int matrix, int full_range, int siting, tg_stream_t stream) {
  TG_REQUIRE(rgb_chw && yuv, TG_E_ARG, "rgb_f32_to_yuv_planar16: null pointer");
  TG_REQUIRE((uintptr_t)yuv % 2 == 0 && (uintptr_t)rgb_chw % 4 == 0, TG_E_ARG,
             "rgb_f32_to_yuv_planar16: yuv is 2-byte aligned and rgb_chw 4-byte aligned");
  TG_REQUIRE(depth == 10 || depth == 12, TG_E_ARG, "rgb_f32_to_yuv_planar16: depth=%d (10 or 12)", depth);
  return tg::rgb_to_yuv_planar<uint16_t>("rgb_f32_to_yuv_planar16", rgb_chw, yuv, n, H, W, chroma, depth, matrix,
                                         full_range, siting, (uintptr_t)rgb_chw % 16 == 0 && (uintptr_t)yuv % 8 == 0,
                                         stream);
}

extern "C" int tg_yuv420p16_to_rgb_f32(const uint16_t* yuv, float* rgb_chw, int n, int h, int w, int depth, int matrix,
                                       int full_range, int siting, tg_stream_t stream) {
  TG_REQUIRE(yuv && rgb_chw, TG_E_ARG, "yuv420p16_to_rgb_f32: null pointer");
  TG_REQUIRE((uintptr_t)yuv % 2 == 0 && (uintptr_t)rgb_chw % 4 == 0, TG_E_ARG,
             "yuv420p16_to_rgb_f32: yuv is 2-byte aligned and rgb_chw 4-byte aligned");
  TG_REQUIRE(depth == 10 || depth == 12, TG_E_ARG, "yuv420p16_to_rgb_f32: depth=%d (10 or 12)", depth);
  TG_REQUIRE(n >= 1 && h >= 2 && w >= 2, TG_E_ARG, "yuv420p16_to_rgb_f32: n=%d h=%d w=%d (n >= 1, h, w >= 2)", n, h, w);
  TG_REQUIRE(tg::yuv_enums_ok(matrix, full_range, siting), TG_E_ARG,
             "yuv420p16_to_rgb_f32: matrix=%d full_range=%d siting=%d", matrix, full_range, siting);
  const int strips = (w + 3) / 4;
  const long long total = (long long)n * h * strips;
  TG_REQUIRE(total < (1LL << 38), TG_E_SHAPE, "yuv420p16_to_rgb_f32: %lld strips", total);
  const bool vec = w % 4 == 0 && (uintptr_t)yuv % 8 == 0 && (uintptr_t)rgb_chw % 16 == 0;
  const tg::yuv_f f = tg::inverse_coefficients_deep(matrix, full_range, depth);
  const int top = (1 << depth) - 1, mid16 = 16 << (depth - 1);
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  const hipStream_t st = (hipStream_t)stream;
#define TG_YUV_IN16(V, L)                                                                                         \
  hipLaunchKernelGGL((tg::yuv420p16_to_rgb_f32_kernel<V, L>), grid, block, 0, st, yuv, rgb_chw, h, w, strips, total, f, \
                     top, mid16)
  if (vec) { if (siting == TG_YUV_LEFT) TG_YUV_IN16(true, true); else TG_YUV_IN16(true, false); }
  else { if (siting == TG_YUV_LEFT) TG_YUV_IN16(false, true); else TG_YUV_IN16(false, false); }
#undef TG_YUV_IN16
  return tg::check_launch("yuv420p16_to_rgb_f32");
}

extern "C" int tg_rgb_f32_to_yuv420p16(const float* rgb_chw, uint16_t* yuv, int n, int H, int W, int depth, int matrix,
                                       int full_range, int siting, tg_stream_t stream) {
  TG_REQUIRE(rgb_chw && yuv, TG_E_ARG, "rgb_f32_to_yuv420p16: null pointer");
  TG_REQUIRE((uintptr_t)yuv % 2 == 0 && (uintptr_t)rgb_chw % 4 == 0, TG_E_ARG,
             "rgb_f32_to_yuv420p16: yuv is 2-byte aligned and rgb_chw 4-byte aligned");
  TG_REQUIRE(depth == 10 || depth == 12, TG_E_ARG, "rgb_f32_to_yuv420p16: depth=%d (10 or 12)", depth);
  TG_REQUIRE(n >= 1 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0, TG_E_ARG,
             "rgb_f32_to_yuv420p16: n=%d H=%d W=%d (n >= 1, H and W even)", n, H, W);
  TG_REQUIRE(tg::yuv_enums_ok(matrix, full_range, siting), TG_E_ARG,
             "rgb_f32_to_yuv420p16: matrix=%d full_range=%d siting=%d", matrix, full_range, siting);
  const int strips = (W + 3) / 4;
  const long long total = (long long)n * (H / 2) * strips;
  TG_REQUIRE(total < (1LL << 38), TG_E_SHAPE, "rgb_f32_to_yuv420p16: %lld strips", total);
  const bool vec = W % 4 == 0 && (uintptr_t)rgb_chw % 16 == 0 && (uintptr_t)yuv % 8 == 0;
  const tg::yuv_q24 q = tg::Q24_TABLE[depth == 12][matrix][full_range];
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  const hipStream_t st = (hipStream_t)stream;
#define TG_YUV_OUT16(V, L)                                                                                        \
  hipLaunchKernelGGL((tg::rgb_f32_to_yuv420p16_kernel<V, L>), grid, block, 0, st, rgb_chw, yuv, H, W, strips, total, q)
  if (vec) { if (siting == TG_YUV_LEFT) TG_YUV_OUT16(true, true); else TG_YUV_OUT16(true, false); }
  else { if (siting == TG_YUV_LEFT) TG_YUV_OUT16(false, true); else TG_YUV_OUT16(false, false); }
#undef TG_YUV_OUT16
  return tg::check_launch("rgb_f32_to_yuv420p16");
}

extern "C" int tg_yuv420_to_rgb_f32(const uint8_t* yuv, float* rgb_chw, int n, int h, int w, int matrix,
                                    int full_range, int siting, tg_stream_t stream) {
  TG_REQUIRE(yuv && rgb_chw, TG_E_ARG, "yuv420_to_rgb_f32: null pointer");
  TG_REQUIRE(n >= 1 && h >= 2 && w >= 2, TG_E_ARG, "yuv420_to_rgb_f32: n=%d h=%d w=%d (n >= 1, h, w >= 2)", n, h, w);
  TG_REQUIRE(tg::yuv_enums_ok(matrix, full_range, siting), TG_E_ARG,
             "yuv420_to_rgb_f32: matrix=%d full_range=%d siting=%d", matrix, full_range, siting);
  const int strips = (w + 3) / 4;
  const long long total = (long long)n * h * strips;
  TG_REQUIRE(total < (1LL << 38), TG_E_SHAPE, "yuv420_to_rgb_f32: %lld strips", total);
  const bool vec = w % 4 == 0 && (uintptr_t)yuv % 4 == 0 && (uintptr_t)rgb_chw % 16 == 0;
  const tg::yuv_f f = tg::inverse_coefficients(matrix, full_range);
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  const hipStream_t st = (hipStream_t)stream;
#define TG_YUV_IN(V, L) \
  hipLaunchKernelGGL((tg::yuv420_to_rgb_f32_kernel<V, L>), grid, block, 0, st, yuv, rgb_chw, h, w, strips, total, f)
  if (vec) { if (siting == TG_YUV_LEFT) TG_YUV_IN(true, true); else TG_YUV_IN(true, false); }
  else { if (siting == TG_YUV_LEFT) TG_YUV_IN(false, true); else TG_YUV_IN(false, false); }
#undef TG_YUV_IN
  return tg::check_launch("yuv420_to_rgb_f32");
}

extern "C" int tg_rgb_u8_to_yuv420(const uint8_t* rgb_hwc, uint8_t* yuv, int n, int H, int W, int matrix,
                                   int full_range, int siting, tg_stream_t stream) {
  TG_REQUIRE(rgb_hwc && yuv, TG_E_ARG, "rgb_u8_to_yuv420: null pointer");
  TG_REQUIRE(n >= 1 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0, TG_E_ARG,
             "rgb_u8_to_yuv420: n=%d H=%d W=%d (n >= 1, H and W even)", n, H, W);
  TG_REQUIRE(tg::yuv_enums_ok(matrix, full_range, siting), TG_E_ARG,
             "rgb_u8_to_yuv420: matrix=%d full_range=%d siting=%d", matrix, full_range, siting);
  const int strips = (W + 3) / 4;
  const long long total = (long long)n * (H / 2) * strips;
  TG_REQUIRE(total < (1LL << 38), TG_E_SHAPE, "rgb_u8_to_yuv420: %lld strips", total);
  const bool vec = W % 4 == 0 && (uintptr_t)rgb_hwc % 4 == 0 && (uintptr_t)yuv % 4 == 0;
  const tg::yuv_q q = tg::Q_TABLE[matrix][full_range];
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  const hipStream_t st = (hipStream_t)stream;
#define TG_YUV_OUT(V, L) \
  hipLaunchKernelGGL((tg::rgb_u8_to_yuv420_kernel<V, L>), grid, block, 0, st, rgb_hwc, yuv, H, W, strips, total, q)
  if (vec) { if (siting == TG_YUV_LEFT) TG_YUV_OUT(true, true); else TG_YUV_OUT(true, false); }
  else { if (siting == TG_YUV_LEFT) TG_YUV_OUT(false, true); else TG_YUV_OUT(false, false); }
#undef TG_YUV_OUT
  return tg::check_launch("rgb_u8_to_yuv420");
}
