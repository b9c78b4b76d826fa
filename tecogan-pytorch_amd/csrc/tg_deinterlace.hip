// Motion-adaptive deinterlacing of planar YUV in front of the stream's YUV launch: interlaced
// frames in, progressive frames at field rate (or one per frame) out, in the same layout and sample type.  The
// specification is tests/deinterlace_ref.py, restated here:
//
//   A frame holds two fields, p = 0 the earlier one.  tff: the earlier field owns the even rows.  par = p ^ (tff ? 0 : 1)
//   is the parity of the rows the field owns.  Y, U and V are treated alike, each with its own ph x pw.
//   owned row (r % 2 == par): cur[r], copied.
//   missing row r: ra = r-1 (r+1 where r-1 < 0), rb = r+1 (r-1 where r+1 >= ph), a = cur[ra], b = cur[rb], every x
//     index clamped into [0, pw-1].  For d in the order 0, -1, +1: score_d = sum_{e in -1,0,1} |a[x+d+e] - b[x-d+e]|,
//     candidate (a[x+d] + b[x-d] + 1) >> 1; sp = the candidate of the smallest score, a later d only on a strictly
//     smaller one.  No frame before (has_prev == 0 and the clip's first frame): out = sp.  Else tp = the sample at (r, x)
//     of the field one back in time (cur[r] for p = 1, prev[r] for p = 0), m = max(|a[x] - prev[ra][x]|,
//     |b[x] - prev[rb][x]|), out = min(max(sp, tp - m), tp + m).
//   Exact integers, no parameters; a 16-bit word above 2^depth - 1 is read as 2^depth - 1, owned rows included.
//
// Thread map.  ONE launch: grid = (pieces of a plane's row pairs / 256, output frames, 3 planes).  A thread makes one
// piece of NS = 16 bytes' worth of samples (16 at 8 bits, 8 above) of a row pair: the owned row's piece, which it has
// loaded anyway as the row above or below, and the missing row's next to it.  The output frame and the plane are
// uniform in a workgroup, and so is the form.
//
// Wide form (a plane's bit in `vecmask`, decided per plane by the entry point): pw * sizeof(T), the plane's offset in
// a frame, the frame's bytes and both bases are multiples of 16, so every piece is one 16-byte buffer load / store;
// the two columns either side of a piece come from the two overlapping dwords next to it (clamped at the plane's
// sides by a select, never read across them).  Both buffers are addressed through ONE descriptor each, with 32-bit
// byte offsets (the entry point keeps them below 2 GiB), so a stray offset is dropped by the hardware.
// Element form (every other width or placement): the same map, samples loaded and stored one by one through clamped
// indices; a piece at the right side may be partial.
//
// Traffic per output frame: the field's rows twice (as the row above and the row below, the second time from L2), the
// same-parity field of the frame before once for each of them, the field one back once: about two frames read, one
// written.
#include "tg_common.h"

namespace tg {

struct deint_geom {
  int ph[3], pw[3];         // rows and columns of Y, U, V
  unsigned off[3];          // a plane's first sample in a frame, in samples
  unsigned frame;           // samples of a frame
  int pieces[3];            // pieces of a row, per plane
};

template <typename T> struct deint_pack;
template <> struct deint_pack<uint8_t> {
  static constexpr int NS = 16;
  static __device__ __forceinline__ void unpack(u32x4 v, int* s) {
#pragma unroll
    for (int i = 0; i < 16; ++i) s[i] = (int)((v[i / 4] >> (8 * (i % 4))) & 255u);
  }
  static __device__ __forceinline__ u32x4 pack(const int* s) {
    u32x4 v;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      v[q] = (unsigned)s[4 * q] | ((unsigned)s[4 * q + 1] << 8) | ((unsigned)s[4 * q + 2] << 16) | ((unsigned)s[4 * q + 3] << 24);
    return v;
  }
  // the last two samples of a dword, and the first two
  static __device__ __forceinline__ void last2(unsigned d, int* s) { s[0] = (int)((d >> 16) & 255u); s[1] = (int)(d >> 24); }
  static __device__ __forceinline__ void first2(unsigned d, int* s) { s[0] = (int)(d & 255u); s[1] = (int)((d >> 8) & 255u); }
};
template <> struct deint_pack<uint16_t> {
  static constexpr int NS = 8;
  static __device__ __forceinline__ void unpack(u32x4 v, int* s) {
#pragma unroll
    for (int i = 0; i < 8; ++i) s[i] = (int)((v[i / 2] >> (16 * (i % 2))) & 65535u);
  }
  static __device__ __forceinline__ u32x4 pack(const int* s) {
    u32x4 v;
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = (unsigned)s[2 * q] | ((unsigned)s[2 * q + 1] << 16);
    return v;
  }
  static __device__ __forceinline__ void last2(unsigned d, int* s) { s[0] = (int)(d & 65535u); s[1] = (int)(d >> 16); }
  static __device__ __forceinline__ void first2(unsigned d, int* s) { s[0] = (int)(d & 65535u); s[1] = (int)(d >> 16); }
};

// What a piece reads and writes.  row(at, x0, s): NS samples from sample offset `at` + x0 of the input; halo(at, x0, pw,
// s): the NS + 4 samples x0 - 2 .. x0 + NS + 1 of the row at `at`, clamped into the row; put(at, x0, pw, s): NS samples
// to the output.  Offsets are in samples from the base; every sample is bounded by `top`.
template <typename T, bool VEC> struct deint_io;

template <typename T> struct deint_io<T, true> {
  typedef deint_pack<T> P;
  static constexpr int NS = P::NS;
  __amdgpu_buffer_rsrc_t in, out;
  int top;
  __device__ __forceinline__ void bound(int* s, int n) const {
    if (sizeof(T) == 2) {
#pragma unroll
      for (int i = 0; i < n; ++i) s[i] = s[i] > top ? top : s[i];
    }
  }
  __device__ __forceinline__ void row(unsigned at, int x0, int, int* s) const {
    P::unpack(buf_ld<u32x4>(in, (at + (unsigned)x0) * (unsigned)sizeof(T)), s);
    bound(s, NS);
  }
  __device__ __forceinline__ void halo(unsigned at, int x0, int pw, int* s) const {
    const unsigned o = (at + (unsigned)x0) * (unsigned)sizeof(T);
    const bool l = x0 > 0, r = x0 + NS < pw;
    const u32x4 mid = buf_ld<u32x4>(in, o);
    const unsigned lo = buf_ld<unsigned>(in, l ? o - 4u : BUF_OOB);
    const unsigned hi = buf_ld<unsigned>(in, r ? o + 16u : BUF_OOB);
    P::unpack(mid, s + 2);
    P::last2(lo, s);
    P::first2(hi, s + NS + 2);
    if (!l) s[0] = s[1] = s[2];
    if (!r) s[NS + 2] = s[NS + 3] = s[NS + 1];
    bound(s, NS + 4);
  }
  __device__ __forceinline__ void put(unsigned at, int x0, int, const int* s) const {
    buf_st(P::pack(s), out, (at + (unsigned)x0) * (unsigned)sizeof(T));
  }
};

template <typename T> struct deint_io<T, false> {
  static constexpr int NS = deint_pack<T>::NS;
  const T* in;
  T* out;
  int top;
  __device__ __forceinline__ int get(unsigned at, int x, int pw) const {
    x = x < 0 ? 0 : (x > pw - 1 ? pw - 1 : x);
    const int v = (int)in[(size_t)at + (size_t)x];
    return sizeof(T) == 1 ? v : (v > top ? top : v);
  }
  __device__ __forceinline__ void row(unsigned at, int x0, int pw, int* s) const {
#pragma unroll
    for (int i = 0; i < NS; ++i) s[i] = get(at, x0 + i, pw);
  }
  __device__ __forceinline__ void halo(unsigned at, int x0, int pw, int* s) const {
#pragma unroll
    for (int i = 0; i < NS + 4; ++i) s[i] = get(at, x0 - 2 + i, pw);
  }
  __device__ __forceinline__ void put(unsigned at, int x0, int pw, const int* s) const {
#pragma unroll
    for (int i = 0; i < NS; ++i)
      if (x0 + i < pw) out[(size_t)at + (size_t)(x0 + i)] = (T)s[i];
  }
};

__device__ __forceinline__ int absdiff(int a, int b) { return a > b ? a - b : b - a; }

// One piece of a row pair.  cur, prev, dst: the plane's first sample in the current frame, the frame before and the
// output frame; ro / rm: the owned and the missing row; temporal: there is a frame before; later: p == 1.
template <typename T, bool VEC>
__device__ __forceinline__ void deint_piece(const deint_io<T, VEC>& io, unsigned cur, unsigned prev, unsigned dst, int ph,
                                            int pw, int ro, int rm, int x0, bool temporal, bool later) {
  constexpr int NS = deint_pack<T>::NS;
  const int ra = rm - 1 >= 0 ? rm - 1 : rm + 1, rb = rm + 1 < ph ? rm + 1 : rm - 1;
  const unsigned upw = (unsigned)pw;
  int A[NS + 4], B[NS + 4];                         // columns x0 - 2 .. x0 + NS + 1 of the rows above and below
  io.halo(cur + (unsigned)ra * upw, x0, pw, A);
  io.halo(cur + (unsigned)rb * upw, x0, pw, B);
  io.put(dst + (unsigned)ro * upw, x0, pw, (ro == ra ? A : B) + 2);      // the owned row is one of the two
  int D0[NS + 2], Dm[NS + 2], Dp[NS + 2];           // |a[j+d] - b[j-d]| at j = x0 - 1 .. x0 + NS, d = 0, -1, +1
#pragma unroll
  for (int j = 0; j < NS + 2; ++j) {
    D0[j] = absdiff(A[j + 1], B[j + 1]);
    Dm[j] = absdiff(A[j], B[j + 2]);
    Dp[j] = absdiff(A[j + 2], B[j]);
  }
  int res[NS];
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    int best = D0[i] + D0[i + 1] + D0[i + 2];
    int sp = (A[i + 2] + B[i + 2] + 1) >> 1;
    const int sm = Dm[i] + Dm[i + 1] + Dm[i + 2], sq = Dp[i] + Dp[i + 1] + Dp[i + 2];
    if (sm < best) { best = sm; sp = (A[i + 1] + B[i + 3] + 1) >> 1; }
    if (sq < best) { sp = (A[i + 3] + B[i + 1] + 1) >> 1; }
    res[i] = sp;
  }
  if (temporal) {
    int PA[NS], PB[NS], TP[NS];
    io.row(prev + (unsigned)ra * upw, x0, pw, PA);
    io.row(prev + (unsigned)rb * upw, x0, pw, PB);
    io.row((later ? cur : prev) + (unsigned)rm * upw, x0, pw, TP);
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const int ma = absdiff(A[i + 2], PA[i]), mb = absdiff(B[i + 2], PB[i]);
      const int m = ma > mb ? ma : mb;
      const int lo = TP[i] - m, hi = TP[i] + m;
      int v = res[i] > lo ? res[i] : lo;
      res[i] = v < hi ? v : hi;
    }
  }
  io.put(dst + (unsigned)rm * upw, x0, pw, res);
}

// blockIdx.y = output frame j, blockIdx.z = plane.  frames: the frame before, then the k frames; output j is field
// f = first_field + j * step counted from frames[1].
template <typename T>
__global__ __launch_bounds__(256) void deinterlace_planar_kernel(const T* __restrict__ frames, T* __restrict__ out,
                                                                 deint_geom g, unsigned in_bytes, unsigned out_bytes,
                                                                 int top, int tff, int has_prev, int first_field, int step,
                                                                 int vecmask) {
  constexpr int NS = deint_pack<T>::NS;
  const int pl = (int)blockIdx.z, j = (int)blockIdx.y;
  const int ph = g.ph[pl], pw = g.pw[pl], pieces = g.pieces[pl];
  const unsigned u = blockIdx.x * 256u + threadIdx.x;
  if (u >= (unsigned)(ph / 2) * (unsigned)pieces) return;
  const int piece = (int)(u % (unsigned)pieces), pair = (int)(u / (unsigned)pieces);
  const int f = first_field + j * step, t = 1 + f / 2, p = f & 1;
  const int par = p ^ (tff ? 0 : 1);
  const int ro = 2 * pair + par, rm = 2 * pair + 1 - par, x0 = piece * NS;
  const bool temporal = t > 1 || has_prev != 0;
  const unsigned cur = (unsigned)t * g.frame + g.off[pl], prev = cur - g.frame, dst = (unsigned)j * g.frame + g.off[pl];
  if ((vecmask >> pl) & 1) {
    const deint_io<T, true> io{TG_BUF_RSRC(frames, in_bytes), TG_BUF_RSRC(out, out_bytes), top};
    deint_piece<T, true>(io, cur, prev, dst, ph, pw, ro, rm, x0, temporal, p == 1);
  } else {
    const deint_io<T, false> io{frames, out, top};
    deint_piece<T, false>(io, cur, prev, dst, ph, pw, ro, rm, x0, temporal, p == 1);
  }
}

template <typename T>
static int deinterlace_planar(const T* frames, T* out, int k, int h, int w, int sx, int sy, int depth, int tff,
                              int has_prev, int first_field, int step, int cnt, tg_stream_t stream) {
  constexpr int NS = deint_pack<T>::NS;
  const int ch = h / sy, cw = (w + sx - 1) / sx;
  const long long fs = (long long)h * w + 2LL * ch * cw;
  // 32-bit byte offsets from either base, and one buffer descriptor per side
  TG_REQUIRE(fs * (k + 1) * (long long)sizeof(T) < (1LL << 31) && fs * cnt * (long long)sizeof(T) < (1LL << 31), TG_E_SHAPE,
             "deinterlace_planar: %d + 1 frames in or %d frames out of %lld samples pass 2 GiB", k, cnt, fs);
  deint_geom g;
  g.ph[0] = h; g.pw[0] = w; g.off[0] = 0;
  g.ph[1] = g.ph[2] = ch; g.pw[1] = g.pw[2] = cw;
  g.off[1] = (unsigned)((long long)h * w); g.off[2] = g.off[1] + (unsigned)((long long)ch * cw);
  g.frame = (unsigned)fs;
  const bool base_ok = (uintptr_t)frames % 16 == 0 && (uintptr_t)out % 16 == 0 && (fs * sizeof(T)) % 16 == 0;
  int vecmask = 0;
  unsigned units = 0;
  for (int pl = 0; pl < 3; ++pl) {
    g.pieces[pl] = (g.pw[pl] + NS - 1) / NS;
    if (base_ok && g.pw[pl] % NS == 0 && (g.off[pl] * sizeof(T)) % 16 == 0) vecmask |= 1 << pl;
    const unsigned n = (unsigned)(g.ph[pl] / 2) * (unsigned)g.pieces[pl];
    units = n > units ? n : units;
  }
  TG_REQUIRE(cnt <= 65535, TG_E_SHAPE, "deinterlace_planar: cnt=%d (at most 65535 frames a call)", cnt);
  const dim3 grid((units + 255u) / 256u, (unsigned)cnt, 3);
  hipLaunchKernelGGL((deinterlace_planar_kernel<T>), grid, dim3(256), 0, (hipStream_t)stream, frames, out, g,
                     (unsigned)(fs * (k + 1) * sizeof(T)), (unsigned)(fs * cnt * sizeof(T)), (1 << depth) - 1, tff, has_prev,
                     first_field, step, vecmask);
  return check_launch("deinterlace_planar");
}

}  // namespace tg

extern "C" int tg_deinterlace_planar(const void* frames, void* out, int k, int h, int w, int chroma, int depth, int tff,
                                     int has_prev, int first_field, int step, int cnt, tg_stream_t stream) {
  TG_REQUIRE(frames && out, TG_E_ARG, "deinterlace_planar: null pointer");
  TG_REQUIRE(depth == 8 || depth == 10 || depth == 12, TG_E_ARG, "deinterlace_planar: depth=%d (8, 10 or 12)", depth);
  TG_REQUIRE(depth == 8 || ((uintptr_t)frames % 2 == 0 && (uintptr_t)out % 2 == 0), TG_E_ARG,
             "deinterlace_planar: 16-bit samples are 2-byte aligned");
  TG_REQUIRE(chroma == TG_YUV_420 || chroma == TG_YUV_422 || chroma == TG_YUV_444, TG_E_ARG,
             "deinterlace_planar: chroma=%d", chroma);
  TG_REQUIRE((tff == 0 || tff == 1) && (has_prev == 0 || has_prev == 1) && (first_field == 0 || first_field == 1) &&
                 (step == 1 || step == 2), TG_E_ARG,
             "deinterlace_planar: tff=%d has_prev=%d first_field=%d (each 0 or 1) step=%d (1 or 2)", tff, has_prev,
             first_field, step);
  const int sx = chroma == TG_YUV_444 ? 1 : 2, sy = chroma == TG_YUV_420 ? 2 : 1;
  TG_REQUIRE(h >= 4 && h % (2 * sy) == 0 && w >= 2, TG_E_ARG,
             "deinterlace_planar: h=%d w=%d (h even and >= 4, a multiple of 4 at 4:2:0; w >= 2)", h, w);
  TG_REQUIRE(k >= 1 && cnt >= 1 && (long long)first_field + (long long)(cnt - 1) * step < 2LL * k, TG_E_ARG,
             "deinterlace_planar: k=%d cnt=%d first_field=%d step=%d (k, cnt >= 1 and the last field inside the k frames)", k,
             cnt, first_field, step);
  if (depth == 8)
    return tg::deinterlace_planar<uint8_t>((const uint8_t*)frames, (uint8_t*)out, k, h, w, sx, sy, depth, tff, has_prev,
                                           first_field, step, cnt, stream);
  return tg::deinterlace_planar<uint16_t>((const uint16_t*)frames, (uint16_t*)out, k, h, w, sx, sy, depth, tff, has_prev,
                                          first_field, step, cnt, stream);
}
