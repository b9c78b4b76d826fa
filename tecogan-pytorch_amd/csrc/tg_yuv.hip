// Planar and semi-planar YUV in and out of the stream (DESIGN.md sections 7e, 7k, 7l, 7p): what a decoder hands over
// and an encoder takes, converted on the device so that fewer bytes cross PCIe than RGB would need.  These are the only
// yuv kernels: ONE template per direction over (sample type T, SX, SY, VEC, LEFT, SEMI), 40 instantiations each, behind
// ten entry points -- the three planar ones, the three semi-planar ones (SEMI) and the four 4:2:0 ones
// (tg_yuv420_to_rgb_f32, tg_rgb_u8_to_yuv420, tg_yuv420p16_to_rgb_f32, tg_rgb_f32_to_yuv420p16), which keep their own
// argument checks (BT.601 / BT.709 only) and launch the planar (2,2) forms.
//
// Format.  A frame is the Y plane H W, then U, then V, each ceil(H/SY) x ceil(W/SX), tightly packed; (SX, SY) is the
// chroma sub-sampling, (2,2) 4:2:0 | (2,1) 4:2:2 | (1,1) 4:4:4.  A sample is a byte at depth 8 (T = uint8_t) and a
// 16-bit little-endian word with d = 10 | 12 significant bits above it (T = uint16_t; one above 2^d - 1 is read as
// 2^d - 1).  LEFT: a chroma sample sits on the left luma column of its pair, else in the centre (along x only; the
// vertical rule of 4:2:0 is the centred one either way).
// SEMI (NV12 / NV16 / NV24, P010 / P012 and their 4:2:2 and 4:4:4 siblings): behind the Y plane ONE chroma plane of
// ceil(H/SY) rows of 2 ceil(W/SX) samples, sample 2c of a row U[r, c] and 2c + 1 V[r, c]; a 16-bit word holds
// code << (16 - d).  It is read as word >> (16 - d) -- nothing exceeds 2^d - 1, the clamp above has nothing to do -- and
// written with the low bits zero; the shift travels as a kernel argument (0 for bytes, not looked at without SEMI).
// Nothing else differs: the values are the planar form's, relaid.
//
// Arithmetic.  Both tables come from (Kr, Kb) in fp64 on the host and travel as kernel arguments (forward_table,
// inverse_table; tg_yuv_tables shows them to the host).
//   in:  chroma to sixteenths in exact integers -- (1,3)/(3,1) around a centred sample, (4)/(2,2) along a co-sited
//        axis, times 4 along an axis that is not sub-sampled, every index clamped into the plane -- then ONE fp32 matrix
//        step and the clamp to [0,1]: no uint8 RGB in between.  The same for both sample types.
//   out: exact integers; the specification is the integer formula itself, which tests/yuv_ref.py, yuv_depth_ref.py and
//        yuv_planar_ref.py restate in numpy, and the bytes / words must be equal.  What the sample type decides is
//        yuv_out<T>: uint8_t takes uint8 HWC RGB (what the HR tail writes), Q = rint(M * 2^16), 32-bit accumulators;
//        uint16_t takes the fp32 CHW HR state through ONE float step per value (clamp, times 65535, round half even:
//        quantize16), Q = rint(M_d * 2^24), 64-bit accumulators.  Y = clip((Q_Y.p + (yo << B) + 2^(B-1)) >> B), B = 16 |
//        24; a chroma sample from the tap-weighted RGB sum of its pixels (the pixel | the pair | (1,2,1) over x-1, x,
//        x+1 with x-1 clamped to 0; times two rows at 4:2:0), shifted by B + log2 of the total tap weight, plus mid.
//
// Thread map.  Pure streaming kernels; one row x 4 pixels on the way in (12 floats written), SY rows x 4 pixels on
// the way out, so that a thread owns whole chroma samples (4 / SX per plane); neighbouring lanes touch neighbouring
// runs of every plane.
//
// Alignment of the wide form (VEC), taken only when W % 4 == 0 and the bases are aligned as the entry points test
// (samples: 4 bytes at 8 bit, 8 bytes at 16 bit; fp32: 16 bytes; uint8 RGB: 4 bytes).  In samples, with W = 4 m:
//   row stride W, and a strip's x0 = 4 tx: multiples of 4.  Y plane H W: a multiple of 4.
//   chroma plane ch cw -- 4:2:0 (on the way in ch = ceil(H/2)): ch 2m, even, and two planes ch W, a multiple of 4;
//   4:2:2: H 2m, even, two planes H W; 4:4:4: H W, a multiple of 4 already.
//   So every frame starts a multiple of 4 samples behind the base, U starts a multiple of 4 behind the frame, and V an
//   even number of samples (a multiple of 4 at 4:4:4) behind U.  A strip's chroma run starts at j cw + x0 / SX: even
//   for SX = 2 (cw = 2m, a run of 2 samples), a multiple of 4 for SX = 1 (cw = 4m, a run of 4).
//   Hence: Y runs of 4 samples and 4:4:4 chroma runs of 4 are aligned to 4 samples (a dword at 8 bit, 8 bytes at 16
//   bit), chroma runs of 2 to 2 samples (a 16-bit word / a dword).  fp32 CHW: plane H W and row W are multiples of 4
//   floats, so every float4 is 16-byte aligned; uint8 HWC: row 3W = 12m and 3 x0 = 12 tx, so the three dwords are.
//   SEMI, same bases, W = 4 m.  The chroma plane starts H W = 4 H m samples behind the frame: a multiple of 4.  Its row
//   is 2 cw samples: 4m for SX = 2 (cw = 2m), 8m for SX = 1.  A frame is H W + ch 2 cw: 4:2:0 (ch = ceil(H/2)) 4m (H +
//   ch), 4:2:2 8 H m, 4:4:4 12 H m -- a multiple of 4, and at 4:4:4 with H m odd of nothing more.  A strip's run of
//   2 NC samples starts at j 2 cw + 2 NC tx: 4 (j m + tx) for SX = 2, 8 (j m + tx) for SX = 1.
//   Hence: for SX = 2 the run of 4 samples (u0 v0 u1 v1) is aligned to its own size, ONE store of 4 samples where the
//   planar form has two of 2; for SX = 1 the run of 8 is aligned to 4 samples only (frame and Y plane are 4:4:4's
//   12 H m and 4 H m), TWO stores of 4 samples.  On the way in the wide loads are the Y samples' (aligned as above: the
//   frame is a multiple of 4 samples for odd h as well); the chroma loads are element-wide in both layouts.
// Every other shape or placement (W = 2 mod 4, odd sizes, a base off its alignment) takes the element-wide form of
// the same kernel.
//
// Compiler note.  clip(acc >> sh, 0, top) of a floor shift is written as a clamp of the accumulator followed by a
// logical shift (the same value: a negative acc gives 0, one of (top + 1) << sh or more gives top).  With the clamp
// AFTER the shift hipcc fuses two neighbours into one v_ashr_pk_u8_i32, whose 16-bit result it then packed into the Y
// dword as if the upper half of the register were zero: bytes 2 and 3 of the store came out wrong on the MI355X.
// shift_clip_u8 and shift_clip_top are the only places that clip, so no packed shift can be formed -- in the SEMI form's
// u0 | v0 << 8 | u1 << 16 | v1 << 24, the very pattern, neither: its four values leave those two functions clamped.
#include "tg_common.h"

namespace tg {

struct yuv_f {          // the inverse step on integers: R = ky*(Y-yo) + rv*dv ... with du, dv = C16 - 16 mid (sixteenths)
  float ky, rv, gu, gv, bu;
  int yo;
};

// clip(acc >> sh, 0, 255): clamp first, then a logical shift (the compiler note above)
__device__ __forceinline__ int shift_clip_u8(int acc, int sh) {
  const int top = (256 << sh) - 1;
  acc = acc < 0 ? 0 : (acc > top ? top : acc);
  return (int)((unsigned)acc >> sh);
}
__device__ __forceinline__ int dot3(const int q[3], const int p[3]) { return q[0] * p[0] + q[1] * p[1] + q[2] * p[2]; }
__device__ __forceinline__ float clamp01(float v) { return __builtin_fminf(__builtin_fmaxf(v, 0.f), 1.f); }

static bool yuv_enums_ok(int matrix, int full_range, int siting) {
  return (matrix == TG_YUV_BT601 || matrix == TG_YUV_BT709) && (full_range == 0 || full_range == 1) &&
         (siting == TG_YUV_CENTER || siting == TG_YUV_LEFT);
}

// the one float step of the output direction: v < 0 and NaN give 0 (both comparisons are false for a NaN, so the first
// one decides), v > 1 gives 65535; one fp32 multiply, one round half even
__device__ __forceinline__ int quantize16(float v) {
  v = v > 0.f ? v : 0.f;
  v = v < 1.f ? v : 1.f;
  return (int)__builtin_rintf(v * 65535.0f);
}
// clip(acc >> sh, 0, top) on 64 bits, as shift_clip_u8 writes it
__device__ __forceinline__ unsigned shift_clip_top(long long acc, int sh, int top) {
  const long long lim = ((long long)(top + 1) << sh) - 1;
  acc = acc < 0 ? 0 : (acc > lim ? lim : acc);
  return (unsigned)((unsigned long long)acc >> sh);
}
__device__ __forceinline__ long long dot3_64(const int q[3], const int p[3]) {
  return (long long)q[0] * p[0] + (long long)q[1] * p[1] + (long long)q[2] * p[2];
}

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

// yo, ys, cs, mid at `depth` bits
static void yuv_scales(int depth, int full_range, int* yo, double* ys, double* cs, int* mid) {
  const int up = depth - 8;
  const double top = (double)((1 << depth) - 1);
  *yo = full_range ? 0 : 16 << up;
  *ys = full_range ? top : (double)(219 << up);
  *cs = full_range ? top : (double)(224 << up);
  *mid = 128 << up;
}

// Q in fp64, rounded half even (the default rounding mode): from RGB levels 0..255 times 2^16 at depth 8, from 16-bit
// codes 0..65535 times 2^24 above.  DESIGN.md sections 7e, 7k and 7l print what this yields.
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

static yuv_f inverse_table(int matrix, int full_range, int depth) {       // the five fp32 gains of the one matrix step
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
// SEMI: the chroma samples of the strip go out as one interleaved run (u0 v0 u1 v1 ...), every sample shifted left by shl.
template <typename T, int SX, int SY, bool VEC, bool LEFT, bool SEMI>
__global__ __launch_bounds__(256) void rgb_to_yuv_planar_kernel(const typename yuv_out<T>::src_t* __restrict__ rgb,
                                                                T* __restrict__ yuv, int H, int W, int strips,
                                                                long long total, yuv_qp q, int shl) {
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
    for (int x = 0; x < 4; ++x) {
      yv[x] = O::clip(O::dot(q.y, p[rr][x]) + yround, O::BASE, q.top);
      if (SEMI) yv[x] <<= shl;
    }
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
  if (SEMI) {                                                     // one run of 2 NC samples, 2 co behind the Y plane
    unsigned cv[2 * NC];
#pragma unroll
    for (int c2 = 0; c2 < NC; ++c2) {
      cv[2 * c2] = uo[c2] << shl;
      cv[2 * c2 + 1] = vo[c2] << shl;
    }
    store_samples<VEC, 4>(up + 2 * co, cv, 2 * ncs);
    if (NC == 4) store_samples<VEC, 4>(up + 2 * co + 4, cv + (NC == 4 ? 4 : 0), 2 * ncs - 4);
  } else {
    store_samples<VEC, NC>(up + co, uo, ncs);
    store_samples<VEC, NC>(vp + co, vo, ncs);
  }
}

// thread = row y x pixels 4*tx .. 4*tx+3 of frame k.  `top` = 2^d - 1 bounds every 16-bit
// sample, `mid16` = 16 * mid.  Along a sub-sampled axis the taps are the ones above; along one that is not, the sample
// of the pixel itself times 4.  Every chroma index is clamped into the plane, so the loads of the pixels past the
// width are in bounds too.
// SEMI: U and V of chroma column c are samples 2c and 2c + 1 of the one chroma plane, and every sample is read as
// word >> shr (element-wide chroma loads in either layout; the wide loads are the Y samples').
template <typename T, int SX, int SY, bool VEC, bool LEFT, bool SEMI>
__global__ __launch_bounds__(256) void yuv_planar_to_rgb_f32_kernel(const T* __restrict__ yuv, float* __restrict__ rgb,
                                                                    int h, int w, int strips, long long total, yuv_f f,
                                                                    int top, int mid16, int shr) {
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
  const T* vp = SEMI ? up + 1 : up + (long long)ch * cw;
  auto sample = [top, shr](const T* p, long long at) {
    const int s = SEMI ? (int)p[2 * at] >> shr : (int)p[at];
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
  if (SEMI) {
#pragma unroll
    for (int x = 0; x < 4; ++x) yy[x] >>= shr;
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

template <typename T, int SX, int SY, bool SEMI>
static void launch_planar_out(bool vec, bool left, dim3 grid, hipStream_t st, const typename yuv_out<T>::src_t* rgb,
                              T* yuv, int H, int W, int strips, long long total, const yuv_qp& q, int shl) {
  constexpr bool L = SX == 2;                                     // (4:4:4 has the one form: the siting is not looked at)
  const dim3 block(256);
  if (vec) {
    if (left) hipLaunchKernelGGL((rgb_to_yuv_planar_kernel<T, SX, SY, true, L, SEMI>), grid, block, 0, st, rgb, yuv, H, W, strips, total, q, shl);
    else hipLaunchKernelGGL((rgb_to_yuv_planar_kernel<T, SX, SY, true, false, SEMI>), grid, block, 0, st, rgb, yuv, H, W, strips, total, q, shl);
  } else {
    if (left) hipLaunchKernelGGL((rgb_to_yuv_planar_kernel<T, SX, SY, false, L, SEMI>), grid, block, 0, st, rgb, yuv, H, W, strips, total, q, shl);
    else hipLaunchKernelGGL((rgb_to_yuv_planar_kernel<T, SX, SY, false, false, SEMI>), grid, block, 0, st, rgb, yuv, H, W, strips, total, q, shl);
  }
}

template <typename T, int SX, int SY, bool SEMI>
static void launch_planar_in(bool vec, bool left, dim3 grid, hipStream_t st, const T* yuv, float* rgb, int h, int w,
                             int strips, long long total, const yuv_f& f, int top, int mid16, int shr) {
  constexpr bool L = SX == 2;
  const dim3 block(256);
  if (vec) {
    if (left) hipLaunchKernelGGL((yuv_planar_to_rgb_f32_kernel<T, SX, SY, true, L, SEMI>), grid, block, 0, st, yuv, rgb, h, w, strips, total, f, top, mid16, shr);
    else hipLaunchKernelGGL((yuv_planar_to_rgb_f32_kernel<T, SX, SY, true, false, SEMI>), grid, block, 0, st, yuv, rgb, h, w, strips, total, f, top, mid16, shr);
  } else {
    if (left) hipLaunchKernelGGL((yuv_planar_to_rgb_f32_kernel<T, SX, SY, false, L, SEMI>), grid, block, 0, st, yuv, rgb, h, w, strips, total, f, top, mid16, shr);
    else hipLaunchKernelGGL((yuv_planar_to_rgb_f32_kernel<T, SX, SY, false, false, SEMI>), grid, block, 0, st, yuv, rgb, h, w, strips, total, f, top, mid16, shr);
  }
}

// the checks and the launch of the output direction for one sample type and chroma layout; `base_ok` = the wide form's
// base alignments.  Semi-planar words carry their code in the top bits: shl = 16 - depth (0 for bytes).
template <typename T, bool SEMI = false>
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
  const int shl = SEMI && depth > 8 ? 16 - depth : 0;
  if (chroma == TG_YUV_420) launch_planar_out<T, 2, 2, SEMI>(vec, left, grid, st, rgb, yuv, H, W, strips, total, q, shl);
  else if (chroma == TG_YUV_422) launch_planar_out<T, 2, 1, SEMI>(vec, left, grid, st, rgb, yuv, H, W, strips, total, q, shl);
  else launch_planar_out<T, 1, 1, SEMI>(vec, left, grid, st, rgb, yuv, H, W, strips, total, q, shl);
  return check_launch(name);
}

// the launch of the input direction for one sample type; the entry points have checked the arguments
template <typename T, bool SEMI = false>
static int yuv_planar_to_rgb(const char* name, const T* yuv, float* rgb, int n, int h, int w, int chroma, int depth,
                             int matrix, int full_range, int siting, bool base_ok, tg_stream_t stream) {
  const int sx = chroma == TG_YUV_444 ? 1 : 2;
  const int strips = (w + 3) / 4;
  const long long total = (long long)n * h * strips;
  TG_REQUIRE(total < (1LL << 38), TG_E_SHAPE, "%s: %lld strips", name, total);
  const bool vec = w % 4 == 0 && base_ok, left = siting == TG_YUV_LEFT && sx == 2;
  const yuv_f f = inverse_table(matrix, full_range, depth);
  const int top = (1 << depth) - 1, mid16 = 16 << (depth - 1);
  const dim3 grid((unsigned)((total + 255) / 256));
  const hipStream_t st = (hipStream_t)stream;
  const int shr = SEMI && depth > 8 ? 16 - depth : 0;
  if (chroma == TG_YUV_420) launch_planar_in<T, 2, 2, SEMI>(vec, left, grid, st, yuv, rgb, h, w, strips, total, f, top, mid16, shr);
  else if (chroma == TG_YUV_422) launch_planar_in<T, 2, 1, SEMI>(vec, left, grid, st, yuv, rgb, h, w, strips, total, f, top, mid16, shr);
  else launch_planar_in<T, 1, 1, SEMI>(vec, left, grid, st, yuv, rgb, h, w, strips, total, f, top, mid16, shr);
  return check_launch(name);
}

// the three entry points of a chroma layout: one body each, the planar and the semi-planar function differ in SEMI and
// in the name their messages carry
template <bool SEMI>
static int yuv_to_rgb_f32_entry(const char* name, const void* yuv, float* rgb_chw, int n, int h, int w, int chroma,
                                int depth, int matrix, int full_range, int siting, tg_stream_t stream) {
  TG_REQUIRE(yuv && rgb_chw, TG_E_ARG, "%s: null pointer", name);
  TG_REQUIRE(depth == 8 || depth == 10 || depth == 12, TG_E_ARG, "%s: depth=%d (8, 10 or 12)", name, depth);
  TG_REQUIRE((depth == 8 || (uintptr_t)yuv % 2 == 0) && (uintptr_t)rgb_chw % 4 == 0, TG_E_ARG,
             "%s: 16-bit samples are 2-byte aligned and rgb_chw 4-byte aligned", name);
  TG_REQUIRE(n >= 1 && h >= 2 && w >= 2, TG_E_ARG, "%s: n=%d h=%d w=%d (n >= 1, h, w >= 2)", name, n, h, w);
  TG_REQUIRE(yuv_planar_enums_ok(chroma, matrix, full_range, siting), TG_E_ARG,
             "%s: chroma=%d matrix=%d full_range=%d siting=%d", name, chroma, matrix, full_range, siting);
  const bool f16 = (uintptr_t)rgb_chw % 16 == 0;
  if (depth == 8)
    return yuv_planar_to_rgb<uint8_t, SEMI>(name, (const uint8_t*)yuv, rgb_chw, n, h, w, chroma, depth, matrix,
                                            full_range, siting, f16 && (uintptr_t)yuv % 4 == 0, stream);
  return yuv_planar_to_rgb<uint16_t, SEMI>(name, (const uint16_t*)yuv, rgb_chw, n, h, w, chroma, depth, matrix,
                                           full_range, siting, f16 && (uintptr_t)yuv % 8 == 0, stream);
}

template <bool SEMI>
static int rgb_u8_to_yuv_entry(const char* name, const uint8_t* rgb_hwc, uint8_t* yuv, int n, int H, int W, int chroma,
                               int matrix, int full_range, int siting, tg_stream_t stream) {
  TG_REQUIRE(rgb_hwc && yuv, TG_E_ARG, "%s: null pointer", name);
  return rgb_to_yuv_planar<uint8_t, SEMI>(name, rgb_hwc, yuv, n, H, W, chroma, 8, matrix, full_range, siting,
                                          (uintptr_t)rgb_hwc % 4 == 0 && (uintptr_t)yuv % 4 == 0, stream);
}

template <bool SEMI>
static int rgb_f32_to_yuv16_entry(const char* name, const float* rgb_chw, uint16_t* yuv, int n, int H, int W,
                                  int chroma, int depth, int matrix, int full_range, int siting, tg_stream_t stream) {
  TG_REQUIRE(rgb_chw && yuv, TG_E_ARG, "%s: null pointer", name);
  TG_REQUIRE((uintptr_t)yuv % 2 == 0 && (uintptr_t)rgb_chw % 4 == 0, TG_E_ARG,
             "%s: yuv is 2-byte aligned and rgb_chw 4-byte aligned", name);
  TG_REQUIRE(depth == 10 || depth == 12, TG_E_ARG, "%s: depth=%d (10 or 12)", name, depth);
  return rgb_to_yuv_planar<uint16_t, SEMI>(name, rgb_chw, yuv, n, H, W, chroma, depth, matrix, full_range, siting,
                                           (uintptr_t)rgb_chw % 16 == 0 && (uintptr_t)yuv % 8 == 0, stream);
}

}  // namespace tg

extern "C" int tg_yuv_planar_to_rgb_f32(const void* yuv, float* rgb_chw, int n, int h, int w, int chroma, int depth,
                                        int matrix, int full_range, int siting, tg_stream_t stream) {
  return tg::yuv_to_rgb_f32_entry<false>("yuv_planar_to_rgb_f32", yuv, rgb_chw, n, h, w, chroma, depth, matrix,
                                         full_range, siting, stream);
}

extern "C" int tg_rgb_u8_to_yuv_planar(const uint8_t* rgb_hwc, uint8_t* yuv, int n, int H, int W, int chroma,
                                       int matrix, int full_range, int siting, tg_stream_t stream) {
  return tg::rgb_u8_to_yuv_entry<false>("rgb_u8_to_yuv_planar", rgb_hwc, yuv, n, H, W, chroma, matrix, full_range,
                                        siting, stream);
}

extern "C" int tg_rgb_f32_to_yuv_planar16(const float* rgb_chw, uint16_t* yuv, int n, int H, int W, int chroma,
                                          int depth, int matrix, int full_range, int siting, tg_stream_t stream) {
  return tg::rgb_f32_to_yuv16_entry<false>("rgb_f32_to_yuv_planar16", rgb_chw, yuv, n, H, W, chroma, depth, matrix,
                                           full_range, siting, stream);
}

// ---- semi-planar: the same bodies with the chroma layout switched --------------------------------
extern "C" int tg_yuv_semiplanar_to_rgb_f32(const void* yuv, float* rgb_chw, int n, int h, int w, int chroma, int depth,
                                            int matrix, int full_range, int siting, tg_stream_t stream) {
  return tg::yuv_to_rgb_f32_entry<true>("yuv_semiplanar_to_rgb_f32", yuv, rgb_chw, n, h, w, chroma, depth, matrix,
                                        full_range, siting, stream);
}

extern "C" int tg_rgb_u8_to_yuv_semiplanar(const uint8_t* rgb_hwc, uint8_t* yuv, int n, int H, int W, int chroma,
                                           int matrix, int full_range, int siting, tg_stream_t stream) {
  return tg::rgb_u8_to_yuv_entry<true>("rgb_u8_to_yuv_semiplanar", rgb_hwc, yuv, n, H, W, chroma, matrix, full_range,
                                       siting, stream);
}

extern "C" int tg_rgb_f32_to_yuv_semiplanar16(const float* rgb_chw, uint16_t* yuv, int n, int H, int W, int chroma,
                                              int depth, int matrix, int full_range, int siting, tg_stream_t stream) {
  return tg::rgb_f32_to_yuv16_entry<true>("rgb_f32_to_yuv_semiplanar16", rgb_chw, yuv, n, H, W, chroma, depth, matrix,
                                          full_range, siting, stream);
}

// ---- the four 4:2:0 entry points: their own checks (BT.601 / BT.709 only), then the (2,2) forms above ------------------
extern "C" int tg_yuv420p16_to_rgb_f32(const uint16_t* yuv, float* rgb_chw, int n, int h, int w, int depth, int matrix,
                                       int full_range, int siting, tg_stream_t stream) {
  TG_REQUIRE(yuv && rgb_chw, TG_E_ARG, "yuv420p16_to_rgb_f32: null pointer");
  TG_REQUIRE((uintptr_t)yuv % 2 == 0 && (uintptr_t)rgb_chw % 4 == 0, TG_E_ARG,
             "yuv420p16_to_rgb_f32: yuv is 2-byte aligned and rgb_chw 4-byte aligned");
  TG_REQUIRE(depth == 10 || depth == 12, TG_E_ARG, "yuv420p16_to_rgb_f32: depth=%d (10 or 12)", depth);
  TG_REQUIRE(n >= 1 && h >= 2 && w >= 2, TG_E_ARG, "yuv420p16_to_rgb_f32: n=%d h=%d w=%d (n >= 1, h, w >= 2)", n, h, w);
  TG_REQUIRE(tg::yuv_enums_ok(matrix, full_range, siting), TG_E_ARG,
             "yuv420p16_to_rgb_f32: matrix=%d full_range=%d siting=%d", matrix, full_range, siting);
  return tg::yuv_planar_to_rgb<uint16_t>("yuv420p16_to_rgb_f32", yuv, rgb_chw, n, h, w, TG_YUV_420, depth, matrix,
                                         full_range, siting, (uintptr_t)yuv % 8 == 0 && (uintptr_t)rgb_chw % 16 == 0,
                                         stream);
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
  return tg::rgb_to_yuv_planar<uint16_t>("rgb_f32_to_yuv420p16", rgb_chw, yuv, n, H, W, TG_YUV_420, depth, matrix,
                                         full_range, siting, (uintptr_t)rgb_chw % 16 == 0 && (uintptr_t)yuv % 8 == 0,
                                         stream);
}

extern "C" int tg_yuv420_to_rgb_f32(const uint8_t* yuv, float* rgb_chw, int n, int h, int w, int matrix,
                                    int full_range, int siting, tg_stream_t stream) {
  TG_REQUIRE(yuv && rgb_chw, TG_E_ARG, "yuv420_to_rgb_f32: null pointer");
  TG_REQUIRE(n >= 1 && h >= 2 && w >= 2, TG_E_ARG, "yuv420_to_rgb_f32: n=%d h=%d w=%d (n >= 1, h, w >= 2)", n, h, w);
  TG_REQUIRE(tg::yuv_enums_ok(matrix, full_range, siting), TG_E_ARG,
             "yuv420_to_rgb_f32: matrix=%d full_range=%d siting=%d", matrix, full_range, siting);
  return tg::yuv_planar_to_rgb<uint8_t>("yuv420_to_rgb_f32", yuv, rgb_chw, n, h, w, TG_YUV_420, 8, matrix, full_range,
                                        siting, (uintptr_t)yuv % 4 == 0 && (uintptr_t)rgb_chw % 16 == 0, stream);
}

extern "C" int tg_rgb_u8_to_yuv420(const uint8_t* rgb_hwc, uint8_t* yuv, int n, int H, int W, int matrix,
                                   int full_range, int siting, tg_stream_t stream) {
  TG_REQUIRE(rgb_hwc && yuv, TG_E_ARG, "rgb_u8_to_yuv420: null pointer");
  TG_REQUIRE(n >= 1 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0, TG_E_ARG,
             "rgb_u8_to_yuv420: n=%d H=%d W=%d (n >= 1, H and W even)", n, H, W);
  TG_REQUIRE(tg::yuv_enums_ok(matrix, full_range, siting), TG_E_ARG,
             "rgb_u8_to_yuv420: matrix=%d full_range=%d siting=%d", matrix, full_range, siting);
  return tg::rgb_to_yuv_planar<uint8_t>("rgb_u8_to_yuv420", rgb_hwc, yuv, n, H, W, TG_YUV_420, 8, matrix, full_range,
                                        siting, (uintptr_t)rgb_hwc % 4 == 0 && (uintptr_t)yuv % 4 == 0, stream);
}

// host query, no device call: what forward_table (q: Y, Cb, Cr rows, then yo, mid, top) and inverse_table (f: ky, rv, gu,
// gv, bu) hand to the kernels
extern "C" int tg_yuv_tables(int depth, int matrix, int full_range, int q[12], float f[5]) {
  double kr, kb;
  TG_REQUIRE(q && f, TG_E_ARG, "yuv_tables: null pointer");
  TG_REQUIRE((depth == 8 || depth == 10 || depth == 12) && tg::yuv_kr_kb(matrix, &kr, &kb) &&
                 (full_range == 0 || full_range == 1),
             TG_E_ARG, "yuv_tables: depth=%d matrix=%d full_range=%d", depth, matrix, full_range);
  const tg::yuv_qp t = tg::forward_table(matrix, full_range, depth);
  const tg::yuv_f g = tg::inverse_table(matrix, full_range, depth);
  for (int c = 0; c < 3; ++c) {
    q[c] = t.y[c];
    q[3 + c] = t.cb[c];
    q[6 + c] = t.cr[c];
  }
  q[9] = t.yo; q[10] = t.mid; q[11] = t.top;
  f[0] = g.ky; f[1] = g.rv; f[2] = g.gu; f[3] = g.gv; f[4] = g.bu;
  return TG_OK;
}
