// The BI degradation: what scripts/generate_lr_bi.m of the reference does to 8-bit frames --
// im2double, modcrop, imresize(img, 1/s, 'bicubic'), imwrite -- as ONE launch of exact integer arithmetic.
//
// For s in {2, 4} and sizes that are multiples of s, MATLAB's contribution algorithm (cubic kernel a = -0.5 stretched
// by s, normalised weights, indices mirrored with the edge pixel repeated) gives every output pixel the same T = 4s
// weights (bi_half below, over 2^8 and 2^12), which sum to exactly 1.  Output pixel o of an axis reads the pixels s*o - 3s/2 .. + 4s - 1.
// With N the separable integer sum and D = DEN^2 the byte is clamp((2N + D) // 2D, 0, 255): round-half-up on the exact
// value.  tests/bi_ref.py is the specification; the bytes (and the fp32 values k / 255) must be equal.
//
// A workgroup makes TG_BI_TILE_H x TG_BI_TILE_W LR pixels of one frame: it stages the (TH*s + 3s) x (TW*s + 3s) GT
// pixels as bytes in LDS (dword loads of the contiguous HWC rows wherever the tile's columns lie inside the frame and
// the rows keep one alignment; mirrored byte loads at the left and right edges; loads issued in batches), runs the
// vertical pass into int32 (|t| <= 255 * 4800 < 2^21), four byte columns per thread, and the horizontal pass from
// there -- in 64 bits for s = 4, where |N| reaches 255 * 4448^2 > 2^32.  No intermediate leaves the workgroup.
#include <type_traits>

#include "tg_common.h"

namespace tg {

constexpr int BI_TH = TG_BI_TILE_H, BI_TW = TG_BI_TILE_W;

// one half of the symmetric kernel (mirror it for the other half); denominators 2^8 and 2^12
template <int S> __device__ __forceinline__ constexpr int bi_half(int k) {
  constexpr int h2[4] = {-3, -9, 29, 111};
  constexpr int h4[8] = {-7, -45, -75, -49, 93, 399, 745, 987};
  return S == 2 ? h2[k & 3] : h4[k & 7];
}
template <int S> constexpr int bi_log2_den() { return S == 2 ? 8 : 12; }

// MATLAB's aux = [1:n, n:-1:1] with mod(i - 1, 2n): the edge pixel is repeated, as often as the halo needs
__device__ __forceinline__ int bi_mirror(int i, int n) {
  while (i < 0 || i >= n) i = i < 0 ? -1 - i : 2 * n - 1 - i;
  return i;
}

// float32_to_uint8 (data_utils.py:80-87) of one value: clip(rint(v * 255), 0, 255), rint = round-half-even
__device__ __forceinline__ unsigned bi_byte_of(float v) {
  const float q = __builtin_fminf(__builtin_fmaxf(rintf(v * 255.0f), 0.f), 255.f);
  return (unsigned)q;
}

// x: uint8 HWC frames (n, H, W, 3), or with F32IN fp32 NCHW (n, 3, H, W) taken to bytes first.  (hc, wc): the
// modcropped size the mirror works on; (oh, ow): LR size; off: first tap of LR pixel 0 (-3s/2 with mirrored borders,
// +s/2 for the bordered training crops, whose taps never leave the frame).
template <int S, bool F32IN>
__global__ __launch_bounds__(256) void downsample_bi_kernel(const void* __restrict__ xin, uint8_t* __restrict__ y_u8,
                                                            float* __restrict__ y_f32, int H, int W, int hc, int wc,
                                                            int oh, int ow, int off, int tiles_x, int tiles_y,
                                                            int rows_aligned) {
  constexpr int T = 4 * S;
  constexpr int RH = BI_TH * S + 3 * S;               // staged rows
  constexpr int CW = BI_TW * S + 3 * S;               // staged pixels per row
  constexpr int ND = (CW * 3 + 3 + 3) / 4;            // dwords per staged row: CW*3 bytes behind a shift of up to 3
  constexpr int CWS = CW / S;                         // = BI_TW + 3
  __shared__ uint32_t tile[RH * ND];                  // bytes [row][shift + px*3 + ch]
  __shared__ int vbuf[BI_TH * 3 * S * CWS];           // vertical sums [r][ch][px % S][px / S]
  uint8_t* tile8 = reinterpret_cast<uint8_t*>(tile);

  const int tid = threadIdx.x;
  int b = blockIdx.x;
  const int tx = b % tiles_x; b /= tiles_x;
  const int ty = b % tiles_y;
  const long long f = b / tiles_y;
  const int ox0 = tx * BI_TW, oy0 = ty * BI_TH;
  const int x_start = S * ox0 + off, y_start = S * oy0 + off;
  // what this tile's outputs read (a partial tile stages less)
  const int need_rows = (oh - oy0 < BI_TH ? oh - oy0 : BI_TH) * S + 3 * S;
  const int need_cols = (ow - ox0 < BI_TW ? ow - ox0 : BI_TW) * S + 3 * S;

  // mirrored source rows and columns of the staged tile, once per workgroup (always valid indices); they live in
  // vbuf, which the vertical pass fills only after the staging is complete
  static_assert(RH + CW <= 256 && RH + CW <= BI_TH * 3 * S * CWS, "index tables: one thread each, inside vbuf");
  int* rowi = vbuf;
  int* coli = vbuf + RH;
  if (tid < RH) rowi[tid] = bi_mirror(y_start + tid, hc);
  else if (tid - RH < CW) coli[tid - RH] = bi_mirror(x_start + (tid - RH), wc);
  __syncthreads();

  // Staging.  Every form first issues a batch of independent loads into registers and only then writes them to LDS:
  // written as load -> store per element the loop waits for one global round trip per iteration.
  int shift = 0;
  constexpr int TOT = RH * 3 * CW;                    // staged bytes
  if (F32IN) {
    const float* x = static_cast<const float*>(xin) + f * 3LL * H * W;
    constexpr int U = 16;
    for (int base = tid; base < TOT; base += 256 * U) {
      float v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = base + 256 * u;
        const int px = i % CW, t = i / CW, ch = t % 3, rr = t / 3;
        const bool ok = i < TOT && rr < need_rows && px < need_cols;
        v[u] = ok ? x[((long long)ch * H + rowi[ok ? rr : 0]) * W + coli[px]] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = base + 256 * u;
        const int px = i % CW, t = i / CW, ch = t % 3, rr = t / 3;
        if (i < TOT) tile8[rr * (ND * 4) + px * 3 + ch] = (uint8_t)bi_byte_of(v[u]);
      }
    }
  } else {
    const uint8_t* x = static_cast<const uint8_t*>(xin) + f * 3LL * H * W;
    const long long row3 = 3LL * W;
    // dword form: every staged column is a real column (two more to spare for the last dword's overhang) and every
    // row starts at the same offset within a dword (rows_aligned: 3W is a multiple of 4)
    const bool vec = rows_aligned && x_start >= 2 && x_start + CW + 2 <= wc;
    if (vec) {
      shift = (int)((uintptr_t)(x + 3 * x_start) & 3);
      const uint8_t* x0 = x + 3 * x_start - shift;
      constexpr int IT = (RH * ND + 255) / 256;
      uint32_t v[IT];
#pragma unroll
      for (int it = 0; it < IT; ++it) {
        const int i = tid + 256 * it;
        const int q = i % ND, rr = i / ND;
        const bool ok = i < RH * ND && rr < need_rows;
        v[it] = ok ? *reinterpret_cast<const uint32_t*>(x0 + rowi[ok ? rr : 0] * row3 + 4 * q) : 0u;
      }
#pragma unroll
      for (int it = 0; it < IT; ++it) {
        const int i = tid + 256 * it;
        if (i < RH * ND) tile[i] = v[it];
      }
    } else {
      constexpr int U = 8;
      for (int base = tid; base < TOT; base += 256 * U) {
        uint8_t v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int i = base + 256 * u;
          const int cb = i % (3 * CW), rr = i / (3 * CW);
          const int px = cb / 3, ch = cb - 3 * px;
          const bool ok = i < TOT && rr < need_rows && px < need_cols;
          v[u] = ok ? x[rowi[ok ? rr : 0] * row3 + 3 * coli[px] + ch] : (uint8_t)0;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int i = base + 256 * u;
          if (i < TOT) tile8[(i / (3 * CW)) * (ND * 4) + i % (3 * CW)] = v[u];
        }
      }
    }
  }
  __syncthreads();

  // vertical pass: four neighbouring byte columns of one LR row per thread
  for (int i = tid; i < BI_TH * ND; i += 256) {
    const int q = i % ND, r = i / ND;
    int acc[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < T / 2; ++k) {
      const uint32_t a = tile[(S * r + k) * ND + q], c = tile[(S * r + T - 1 - k) * ND + q];
      const int w = bi_half<S>(k);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] += w * (int)(((a >> (8 * e)) & 255u) + ((c >> (8 * e)) & 255u));
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int j = 4 * q + e - shift;                 // px * 3 + ch
      if (j >= 0 && j < 3 * CW) {
        const int px = j / 3, ch = j - 3 * px;
        vbuf[((r * 3 + ch) * S + px % S) * CWS + px / S] = acc[e];
      }
    }
  }
  __syncthreads();

  // horizontal pass, rounding, both outputs: lanes run along the LR row
  constexpr int SH = 2 * bi_log2_den<S>();           // D = 2^SH
  using acc_t = typename std::conditional<S == 4, long long, int>::type;
  for (int i = tid; i < BI_TH * 3 * BI_TW; i += 256) {
    const int oxl = i % BI_TW, t = i / BI_TW, ch = t % 3, r = t / 3;
    const int oy = oy0 + r, ox = ox0 + oxl;
    if (oy >= oh || ox >= ow) continue;
    const int* v = vbuf + (r * 3 + ch) * S * CWS + oxl;
    acc_t N = 0;
#pragma unroll
    for (int k = 0; k < T / 2; ++k) {
      const int k2 = T - 1 - k;
      const int pair = v[(k % S) * CWS + k / S] + v[(k2 % S) * CWS + k2 / S];
      N += (acc_t)bi_half<S>(k) * (acc_t)pair;
    }
    // (2N + D) // 2D = (N + D/2) >> SH, clamped to a byte: clamp first, then a logical shift (tg_yuv.hip's form)
    acc_t a = N + ((acc_t)1 << (SH - 1));
    const acc_t top = ((acc_t)256 << SH) - 1;
    a = a < 0 ? 0 : (a > top ? top : a);
    const unsigned byte = (unsigned)((unsigned long long)a >> SH);
    if (y_u8) y_u8[((f * oh + oy) * ow + ox) * 3 + ch] = (uint8_t)byte;
    if (y_f32) y_f32[((f * 3 + ch) * oh + oy) * ow + ox] = (float)byte / 255.0f;   // what a loader makes of an LR PNG
  }
}

static int downsample_bi_launch(const char* what, const void* x, bool f32in, uint8_t* y_u8, float* y_f32, int n, int h,
                                int w, int scale, int pad, tg_stream_t stream) {
  TG_REQUIRE(x && (y_u8 || y_f32), TG_E_ARG, "%s: null pointer (x and at least one output)", what);
  TG_REQUIRE(scale == 2 || scale == 4, TG_E_ARG, "%s: scale=%d (2 or 4)", what, scale);
  TG_REQUIRE(n >= 1 && h >= scale && w >= scale, TG_E_SHAPE, "%s: n=%d h=%d w=%d (n >= 1, h and w >= scale %d)", what, n,
             h, w, scale);
  const int hc = h - h % scale, wc = w - w % scale;
  TG_REQUIRE(pad || (hc > 4 * scale && wc > 4 * scale), TG_E_SHAPE,
             "%s: pad=0 reads a border of %d pixels per side, h=%d w=%d leave no output", what, 2 * scale, h, w);
  const int cut = pad ? 0 : 4;
  const int oh = hc / scale - cut, ow = wc / scale - cut;
  const int off = pad ? -3 * scale / 2 : scale / 2;
  const int tiles_x = tg::cdiv(ow, BI_TW), tiles_y = tg::cdiv(oh, BI_TH);
  const long long blocks = (long long)tiles_x * tiles_y * n;
  TG_REQUIRE(blocks < (1LL << 31), TG_E_SHAPE, "%s: %lld workgroups", what, blocks);
  const int rows_aligned = w % 4 == 0 ? 1 : 0;
  const dim3 grid((unsigned)blocks), block(256);
  const hipStream_t st = (hipStream_t)stream;
#define TG_BI_GO(S, F) \
  hipLaunchKernelGGL((downsample_bi_kernel<S, F>), grid, block, 0, st, x, y_u8, y_f32, h, w, hc, wc, oh, ow, off, \
                     tiles_x, tiles_y, rows_aligned)
  if (scale == 2) { if (f32in) TG_BI_GO(2, true); else TG_BI_GO(2, false); }
  else { if (f32in) TG_BI_GO(4, true); else TG_BI_GO(4, false); }
#undef TG_BI_GO
  return check_launch(what);
}

}  // namespace tg

extern "C" int tg_downsample_bi_u8(const uint8_t* x_hwc, uint8_t* y_u8_hwc, float* y_f32_chw, int n, int h, int w,
                                   int scale, int pad, tg_stream_t stream) {
  return tg::downsample_bi_launch("downsample_bi_u8", x_hwc, false, y_u8_hwc, y_f32_chw, n, h, w, scale, pad, stream);
}

extern "C" int tg_downsample_bi_f32(const float* x_chw, uint8_t* y_u8_hwc, float* y_f32_chw, int n, int h, int w,
                                    int scale, int pad, tg_stream_t stream) {
  return tg::downsample_bi_launch("downsample_bi_f32", x_chw, true, y_u8_hwc, y_f32_chw, n, h, w, scale, pad, stream);
}
