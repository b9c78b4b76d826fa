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

// ---- bicubic resize to any size, table-driven -------------------------------------------------
// The general case of the kernel above: the weights differ per output pixel, so they come as tables, built on the host
// by the contribution algorithm (tests/resize_ref.py is the specification): per axis idx[n_out][taps] (input pixel,
// already mirrored) and w[n_out][taps] (int16 over 2^14, every row sums to 2^14).  With N the separable integer sum the
// byte is clamp((N + 2^27) >> 28, 0, 255).
//
// A workgroup makes RS_TH x RS_TW output pixels of one frame.  It copies the tile's table rows into LDS, every index
// clamped to [0, n_in - 1]; their minimum and maximum per axis are the tile's input footprint, a plain rectangle of
// the frame (the mirroring is in the tables), at most RS_RH x RS_CW pixels at the ratio 1/4.  The host sizes the LDS by
// what the call's ratios can ask for (resample_tile_span: 13 KB at 3/4, 39 KB at 1/4, 42 KB at most).  The rectangle is staged as
// bytes: aligned dword loads of every row (a dword that reaches past either end of the row's bytes is put together from
// byte loads, so nothing outside the rectangle is read), written to LDS byte by byte so that every staged row starts at
// its first byte whatever its alignment in memory.  Vertical pass on dwords of four byte columns into int32
// (|t| <= 255 * 18 * 2^15 < 2^28 for ANY table), horizontal pass in 64 bits, one rounding.  A table that is wrong gives wrong bytes, never an access outside the frame
// or the staged tile: offsets into the tile are clamped to what was staged.
namespace tg {

constexpr int RS_TH = 8, RS_TW = 32, RS_T = TG_RESAMPLE_MAX_TAPS, RS_SH = 2 * TG_RESAMPLE_WEIGHT_BITS;
constexpr int RS_RH = 50, RS_CW = 146;                // footprint of a tile at 1/4: (T - 1) * 4 + 1 + 18 = 47 and 143

// Pixels along an axis that a tile of `tile` outputs can read: output o's first tap is floor(u_o - kw / 2) with
// u_{o+1} - u_o = n_in / n_out, so two neighbours' first taps lie at most ceil(n_in / n_out) apart; the kept taps are
// among the taps + 2 columns the contribution algorithm starts from; mirroring only folds them back into the frame.
__host__ __device__ inline int resample_tile_span(int n_in, int n_out, int taps, int tile) {
  const long long step = ((long long)n_in + n_out - 1) / n_out;
  const long long v = (tile - 1) * step + taps + 2;
  return (int)(v < n_in ? v : n_in);
}
static_assert((RS_TH - 1) * 4 + RS_T + 2 <= RS_RH && (RS_TW - 1) * 4 + RS_T + 2 <= RS_CW, "the ratio 1/4 fits the caps");

__global__ __launch_bounds__(256) void resample_u8_kernel(const uint8_t* __restrict__ x, uint8_t* __restrict__ y,
                                                          int h_in, int w_in, int h_out, int w_out,
                                                          const int* __restrict__ v_idx, const int16_t* __restrict__ v_w,
                                                          int v_taps, const int* __restrict__ h_idx,
                                                          const int16_t* __restrict__ h_w, int h_taps, int tiles_x,
                                                          int tiles_y, int rh_cap, int cw_cap) {
  // LDS, sized by the host (resample_lds_bytes): the staged tile of rh_cap rows x nd_cap dwords, the vertical sums,
  // the tile's table rows, the footprint
  extern __shared__ __attribute__((aligned(16))) uint32_t rs_lds[];
  const int nd_cap = (cw_cap * 3 + 3) / 4;            // dwords per staged row
  const int vrow = nd_cap * 4;                        // vertical sums per tile row, a multiple of 4
  uint32_t* tile = rs_lds;                            // bytes [row][px * 3 + ch]
  int* vbuf = reinterpret_cast<int*>(rs_lds + (rh_cap * nd_cap + 3) / 4 * 4);   // vertical sums [r][px * 3 + ch], 16-byte aligned
  int* s_vi = vbuf + RS_TH * vrow;                    // first the clamped indices, then offsets into tile / vbuf
  int* s_vw = s_vi + RS_TH * v_taps;
  int* s_hi = s_vw + RS_TH * v_taps;
  int* s_hw = s_hi + RS_TW * h_taps;
  int* s_lim = s_hw + RS_TW * h_taps;                 // row min, row max, column min, column max
  uint8_t* tile8 = reinterpret_cast<uint8_t*>(tile);

  const int tid = threadIdx.x;
  int b = blockIdx.x;
  const int tx = b % tiles_x; b /= tiles_x;
  const int ty = b % tiles_y;
  const long long f = b / tiles_y;
  const int ox0 = tx * RS_TW, oy0 = ty * RS_TH;
  const int th = h_out - oy0 < RS_TH ? h_out - oy0 : RS_TH;
  const int tw = w_out - ox0 < RS_TW ? w_out - ox0 : RS_TW;

  if (tid == 0) { s_lim[0] = h_in - 1; s_lim[1] = 0; s_lim[2] = w_in - 1; s_lim[3] = 0; }
  __syncthreads();
  int lo_v = h_in - 1, hi_v = 0, lo_h = w_in - 1, hi_h = 0;
  for (int i = tid; i < th * v_taps; i += 256) {      // (rows oy0 .. oy0 + th - 1 of a table are contiguous)
    int v = v_idx[(long long)oy0 * v_taps + i];
    v = v < 0 ? 0 : (v > h_in - 1 ? h_in - 1 : v);
    s_vi[i] = v;
    s_vw[i] = (int)v_w[(long long)oy0 * v_taps + i];
    lo_v = v < lo_v ? v : lo_v;
    hi_v = v > hi_v ? v : hi_v;
  }
  for (int i = tid; i < tw * h_taps; i += 256) {
    int v = h_idx[(long long)ox0 * h_taps + i];
    v = v < 0 ? 0 : (v > w_in - 1 ? w_in - 1 : v);
    s_hi[i] = v;
    s_hw[i] = (int)h_w[(long long)ox0 * h_taps + i];
    lo_h = v < lo_h ? v : lo_h;
    hi_h = v > hi_h ? v : hi_h;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {           // the wave's extremes, then one LDS atomic each per wave
    const int a = __shfl_xor(lo_v, off), b2 = __shfl_xor(hi_v, off), c = __shfl_xor(lo_h, off), d = __shfl_xor(hi_h, off);
    lo_v = a < lo_v ? a : lo_v;
    hi_v = b2 > hi_v ? b2 : hi_v;
    lo_h = c < lo_h ? c : lo_h;
    hi_h = d > hi_h ? d : hi_h;
  }
  if ((tid & 63) == 0) {
    atomicMin(&s_lim[0], lo_v);
    atomicMax(&s_lim[1], hi_v);
    atomicMin(&s_lim[2], lo_h);
    atomicMax(&s_lim[3], hi_h);
  }
  __syncthreads();
  const int y_lo = s_lim[0], x_lo = s_lim[2];
  int nr = s_lim[1] - y_lo + 1, nc = s_lim[3] - x_lo + 1;
  nr = nr > rh_cap ? rh_cap : nr;                     // (only a wrong table asks for more)
  nc = nc > cw_cap ? cw_cap : nc;
  const int nc3 = 3 * nc;

  const uint8_t* xf = x + f * 3LL * h_in * w_in + 3 * x_lo;
  const long long row3 = 3LL * w_in;

  // staging: a batch of independent loads into registers, then the LDS writes (as in the kernel above).  A row's
  // shift is where its first byte sits inside its aligned dword in memory.
  const int nd = (nc3 + 3 + 3) / 4;                   // aligned dwords of a row that can hold one of its bytes
  const int tot = nr * nd;
  constexpr int U = 8;
  for (int base = tid; base < tot; base += 256 * U) {
    uint32_t v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = base + 256 * u;
      v[u] = 0u;
      if (i < tot) {
        const int q = i % nd, rr = i / nd;
        const uint8_t* row = xf + (y_lo + rr) * row3;
        const int first = 4 * q - (int)((uintptr_t)row & 3);             // the aligned dword's first byte in the row's nc3
        if (first >= 0 && first + 4 <= nc3) {
          v[u] = *reinterpret_cast<const uint32_t*>(row + first);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (first + e >= 0 && first + e < nc3) v[u] |= (uint32_t)row[first + e] << (8 * e);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = base + 256 * u;
      if (i < tot) {
        const int q = i % nd, rr = i / nd;
        const int first = 4 * q - (int)((uintptr_t)(xf + (y_lo + rr) * row3) & 3);
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (first + e >= 0 && first + e < nc3) tile8[rr * vrow + first + e] = (uint8_t)(v[u] >> (8 * e));
      }
    }
  }
  // indices -> offsets: first dword of the row in the tile; first int of a column's triple in a vbuf row
  for (int i = tid; i < th * v_taps; i += 256) {
    int rel = s_vi[i] - y_lo;
    rel = rel > nr - 1 ? nr - 1 : rel;
    s_vi[i] = rel * nd_cap;
  }
  for (int i = tid; i < tw * h_taps; i += 256) {
    int rel = s_hi[i] - x_lo;
    rel = rel > nc - 1 ? nc - 1 : rel;
    s_hi[i] = 3 * rel;
  }
  __syncthreads();

  // vertical pass: four neighbouring byte columns of one output row per step, lanes along the staged row (the last
  // dword of a row may hold bytes nobody staged: their sums are never read)
  const int nd4 = (nc3 + 3) >> 2;
  for (int i = tid; i < th * nd4; i += 256) {
    const int q = i % nd4, r = i / nd4;
    int acc[4] = {0, 0, 0, 0};
    for (int k = 0; k < v_taps; ++k) {
      const int w = s_vw[r * v_taps + k];
      const uint32_t d = tile[s_vi[r * v_taps + k] + q];
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] += w * (int)((d >> (8 * e)) & 255u);
    }
    *reinterpret_cast<int4*>(vbuf + r * vrow + 4 * q) = make_int4(acc[0], acc[1], acc[2], acc[3]);
  }
  __syncthreads();

  // horizontal pass and the rounding: lanes along the output row's bytes
  const int tw3 = 3 * tw;
  for (int i = tid; i < th * tw3; i += 256) {
    const int j = i % tw3, r = i / tw3;
    const int oxl = j / 3, ch = j - 3 * oxl;
    const int* v = vbuf + r * vrow + ch;
    long long N = 0;
    for (int k = 0; k < h_taps; ++k) N += (long long)s_hw[oxl * h_taps + k] * (long long)v[s_hi[oxl * h_taps + k]];
    // (N + 2^27) >> 28 clamped to a byte: clamp first, then a logical shift (tg_yuv.hip's form)
    long long a = N + (1LL << (RS_SH - 1));
    const long long top = (256LL << RS_SH) - 1;
    a = a < 0 ? 0 : (a > top ? top : a);
    y[((f * h_out + (oy0 + r)) * w_out + ox0) * 3 + j] = (uint8_t)((unsigned long long)a >> RS_SH);
  }
}

// the dynamic LDS of a launch with these caps and tap counts, as the kernel lays it out
static size_t resample_lds_bytes(int rh_cap, int cw_cap, int v_taps, int h_taps) {
  const int nd_cap = (cw_cap * 3 + 3) / 4;
  return 4 * ((size_t)(rh_cap * nd_cap + 3) / 4 * 4 + (size_t)RS_TH * nd_cap * 4 + 2 * (size_t)(RS_TH * v_taps + RS_TW * h_taps) + 4);
}

}  // namespace tg

extern "C" int tg_resample_tile_span(int n_in, int n_out, int taps, int tile) {
  if (n_in < 1 || n_out < 1 || taps < 1 || tile < 1) return -1;
  return tg::resample_tile_span(n_in, n_out, taps, tile);
}

extern "C" int tg_resample_u8(const uint8_t* x_hwc, uint8_t* y_hwc, int n, int h_in, int w_in, int h_out, int w_out,
                              const int32_t* v_idx, const int16_t* v_w, int v_taps, const int32_t* h_idx,
                              const int16_t* h_w, int h_taps, tg_stream_t stream) {
  TG_REQUIRE(x_hwc && y_hwc && v_idx && v_w && h_idx && h_w, TG_E_ARG, "resample_u8: null pointer");
  TG_REQUIRE(n >= 1, TG_E_ARG, "resample_u8: n=%d (n >= 1)", n);
  TG_REQUIRE(v_taps >= 1 && v_taps <= TG_RESAMPLE_MAX_TAPS && h_taps >= 1 && h_taps <= TG_RESAMPLE_MAX_TAPS, TG_E_ARG,
             "resample_u8: v_taps=%d h_taps=%d (1 .. %d)", v_taps, h_taps, TG_RESAMPLE_MAX_TAPS);
  TG_REQUIRE(h_in >= 1 && w_in >= 1 && h_out >= 1 && w_out >= 1, TG_E_SHAPE,
             "resample_u8: %dx%d -> %dx%d (every size >= 1)", h_in, w_in, h_out, w_out);
  TG_REQUIRE(4LL * h_out >= h_in && h_out <= 4LL * h_in && 4LL * w_out >= w_in && w_out <= 4LL * w_in, TG_E_SHAPE,
             "resample_u8: %dx%d -> %dx%d (the ratio of either axis lies in [1/4, 4])", h_in, w_in, h_out, w_out);
  TG_REQUIRE(3LL * h_in * w_in < (1LL << 31) && 3LL * h_out * w_out < (1LL << 31), TG_E_SHAPE,
             "resample_u8: %dx%d -> %dx%d (a frame has fewer than 2^31 bytes)", h_in, w_in, h_out, w_out);
  const int tiles_x = tg::cdiv(w_out, tg::RS_TW), tiles_y = tg::cdiv(h_out, tg::RS_TH);
  const long long blocks = (long long)tiles_x * tiles_y * n;
  TG_REQUIRE(blocks < (1LL << 31), TG_E_SHAPE, "resample_u8: %lld workgroups", blocks);
  // what a tile can read at these ratios, never more than the caps: a table that asks for more is clamped to them
  const int rh = tg::resample_tile_span(h_in, h_out, v_taps, tg::RS_TH), cw = tg::resample_tile_span(w_in, w_out, h_taps, tg::RS_TW);
  const int rh_cap = rh < tg::RS_RH ? rh : tg::RS_RH, cw_cap = cw < tg::RS_CW ? cw : tg::RS_CW;
  const size_t lds = tg::resample_lds_bytes(rh_cap, cw_cap, v_taps, h_taps);
  hipLaunchKernelGGL(tg::resample_u8_kernel, dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, x_hwc, y_hwc,
                     h_in, w_in, h_out, w_out, v_idx, v_w, v_taps, h_idx, h_w, h_taps, tiles_x, tiles_y, rh_cap, cw_cap);
  return tg::check_launch("resample_u8");
}
