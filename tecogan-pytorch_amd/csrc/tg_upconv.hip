// conv3x3(bilinear_x2(x)) with the matrix work at the LOW resolution ("Up-sampling readers").
//
// Up-sampling acts per channel and a conv tap's channel mix acts per pixel, so the two commute:
//   conv3x3(up2(x))[o, Y, X] = b[o] + sum over (ky, kx) of inside(Y+ky-1, X+kx-1) * up2(z[ky, kx, o])[Y+ky-1, X+kx-1]
//   z[ky, kx, o][a, b]       = sum over c of W[o, c, ky, kx] * x[c, a, b]
// Two plain data-parallel launches, no workgroup waits for another, no atomics:
//   tap GEMM   z[img] (9 cout x h w) = A (9 cout x cin, tg_upconv_pack) * x[img] (cin x h w), fp32 MFMA 32x32x2, a quarter
//              of the direct form's multiplies; no bias, no halo, no transform;
//   combine    y = act(bias + the nine shifted, up-sampled z planes): a low-resolution tile of the nine planes with its
//              clamped one-pixel halo in LDS, blended along x, then along y (about 15 multiply-adds per output, not 36).
// FNet's three readers of a decoder block (tecogan_nets.py:44-64): cin 256 / 128 / 64, cout = cin / 2.
#include "tg_common.h"

namespace tg {

// ---- tap GEMM -------------------------------------------------------------------------------------------------------
// One workgroup (4 waves): 128 pixels x 96 rows of A (3 MFMA tiles of 32), K in chunks of 32 channels through LDS.
// The MFMA's first operand is x^T (pixel on the lane, so the four consecutive accumulator registers of a lane are
// four consecutive pixels: one 16-byte store), its second A^T in the packed order [m / 32][k / 2][lane].
constexpr int UG_PX = 128, UG_M = 96, UG_K = 32, UG_MT = UG_M / 32;

struct UpGemmArgs {
  const float *x, *a;
  float* z;
  int64_t x_ns, z_ns;
  int cin, m, hw;      // m = 9 * cout
};

template <bool VEC>
__global__ __launch_bounds__(256) void upconv_tap_gemm_kernel(UpGemmArgs g) {
  __shared__ float lds[UG_K * UG_PX + UG_MT * (UG_K / 2) * 64];
  float* const xs = lds;                      // [UG_K][UG_PX]
  float* const as = lds + UG_K * UG_PX;       // [UG_MT][UG_K / 2][64]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int p0 = blockIdx.x * UG_PX, mt0 = blockIdx.y * UG_MT, img = blockIdx.z;
  const int hw = g.hw, k2n = g.cin / 2;
  const __amdgpu_buffer_rsrc_t xr = TG_BUF_RSRC(g.x + img * g.x_ns, (unsigned)g.cin * hw * 4u);
  const __amdgpu_buffer_rsrc_t ar = TG_BUF_RSRC(g.a, (unsigned)g.m * g.cin * 4u);
  const __amdgpu_buffer_rsrc_t zr = TG_BUF_RSRC(g.z + img * g.z_ns, (unsigned)g.m * hw * 4u);

  f32x4 xv[4], av[UG_MT];
  auto fetch = [&](int k0) {
    if constexpr (VEC) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int idx = tid + i * 256, row = idx >> 5, px = p0 + (idx & 31) * 4;
        xv[i] = buf_ld<f32x4>(xr, px < hw ? (unsigned)((k0 + row) * hw + px) * 4u : BUF_OOB);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int idx = tid + (i * 4 + j) * 256, row = idx >> 7, px = p0 + (idx & 127);
          xv[i][j] = buf_ld<float>(xr, px < hw ? (unsigned)((k0 + row) * hw + px) * 4u : BUF_OOB);
        }
    }
#pragma unroll
    for (int t = 0; t < UG_MT; ++t)
      av[t] = buf_ld<f32x4>(ar, (unsigned)(((mt0 + t) * k2n + k0 / 2) * 64 + tid * 4) * 4u);
  };
  auto stage = [&] {
    if constexpr (VEC) {
#pragma unroll
      for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(xs + (tid + i * 256) * 4) = xv[i];
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) xs[tid + (i * 4 + j) * 256] = xv[i][j];
    }
#pragma unroll
    for (int t = 0; t < UG_MT; ++t) *reinterpret_cast<f32x4*>(as + t * (UG_K / 2) * 64 + tid * 4) = av[t];
  };

  f32x16 acc[UG_MT];
#pragma unroll
  for (int t = 0; t < UG_MT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  fetch(0);
  for (int k0 = 0; k0 < g.cin; k0 += UG_K) {
    stage();
    __syncthreads();
    if (k0 + UG_K < g.cin) fetch(k0 + UG_K);      // in flight behind this chunk's products
    const float* xl = xs + (lane >> 5) * UG_PX + wv * 32 + (lane & 31);
#pragma unroll
    for (int kk = 0; kk < UG_K / 2; ++kk) {
      const float xa = xl[kk * 2 * UG_PX];
#pragma unroll
      for (int t = 0; t < UG_MT; ++t)
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa, as[(t * (UG_K / 2) + kk) * 64 + lane], acc[t], 0, 0, 0);
    }
    __syncthreads();
  }

  // accumulator register r of a lane: pixel (r & 3) + 8 (r >> 2) + 4 (lane >> 5) of the wave's 32, row lane & 31 of the tile
#pragma unroll
  for (int t = 0; t < UG_MT; ++t) {
    const unsigned mrow = (unsigned)((mt0 + t) * 32 + (lane & 31)) * (unsigned)hw;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int px = p0 + wv * 32 + 8 * q + 4 * (lane >> 5);
      if constexpr (VEC) {
        const f32x4 v = {acc[t][4 * q], acc[t][4 * q + 1], acc[t][4 * q + 2], acc[t][4 * q + 3]};
        buf_st(v, zr, px < hw ? (mrow + px) * 4u : BUF_OOB);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) buf_st(acc[t][4 * q + j], zr, px + j < hw ? (mrow + px + j) * 4u : BUF_OOB);
      }
    }
  }
}

// A in the order a lane consumes it: out[m / 32][k / 2][lane] = W[o][c = 2 (k / 2) + lane / 32][tap], m = tap * cout + o
// = 32 (m / 32) + lane % 32.  ocb 0: w is OIHW; 32 / 64: w is tg_conv3x3_pack's [ocg][chunk][tap][half][ocb][4].
__global__ void upconv_pack_kernel(const float* __restrict__ w, float* __restrict__ out, int cin, int cout, int ocb) {
  const int total = 9 * cout * cin, k2n = cin / 2, nchunk = cdiv(cin, CK);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int lane = i & 63, k2 = (i >> 6) % k2n, mt = (i >> 6) / k2n;
    const int m = mt * 32 + (lane & 31), c = 2 * k2 + (lane >> 5), tap = m / cout, o = m % cout;
    size_t src;
    if (ocb == 0) src = ((size_t)o * cin + c) * 9 + tap;
    else src = (((((size_t)(o / ocb) * nchunk + c / CK) * 9 + tap) * 2 + (c % CK) / 4) * ocb + o % ocb) * 4 + c % 4;
    out[i] = w[src];
  }
}

// ---- combine --------------------------------------------------------------------------------------------------------
// One workgroup: one output channel of one image, a UC_H x UC_W tile of the low-resolution map -> 2 UC_H x 2 UC_W outputs.
// bilinear x2, align_corners = False: up[2a] = 1/4 v[a-1] + 3/4 v[a], up[2a+1] = 3/4 v[a] + 1/4 v[a+1], indices clamped
// (bilinear_src gives the same taps and weights); the clamp is made once, where the halo is staged.
// A thread blends one low-resolution pixel's two output columns along x (7 staged values), then one low-resolution
// row's two output rows of four columns along y (7 float4 of the x-blended rows).
constexpr int UC_H = 16, UC_W = 32, UC_ZH = UC_H + 2, UC_ZW = UC_W + 2;
static_assert(UC_H * (2 * UC_W / 4) == 256 && UC_W == 32, "the combine's thread maps");

struct UpCombineArgs {
  const float *z, *bias;
  float* y;
  int64_t z_ns, y_ns;
  int cout, h, w, act, tiles_x;      // h, w: the low-resolution map
};

// the sample of the x2 up-sampling that lies between the neighbours m and c, a quarter of the way from c
__device__ __forceinline__ float near_c(float m, float c) { return 0.25f * m + 0.75f * c; }
__device__ __forceinline__ f32x4 near_c(f32x4 m, f32x4 c) { return 0.25f * m + 0.75f * c; }

template <bool VEC>
__global__ __launch_bounds__(256) void upconv_combine_kernel(UpCombineArgs g) {
  // both arrays end in the rows of the loops' last, partly idle round of eight (filled, never read)
  constexpr int ZROWS = 9 * UC_ZH, ZROUNDS = (ZROWS + 7) / 8, HROWS = 3 * UC_ZH, HROUNDS = (HROWS + 7) / 8;
  __shared__ float zs[ZROUNDS * 8 * UC_ZW];                                   // [tap][low row + halo][low column + halo]
  __shared__ __attribute__((aligned(16))) float hx[HROUNDS * 8 * 2 * UC_W];   // [ky][low row + halo][output column]
  const int tid = threadIdx.x, col = tid & 31, rgrp = tid >> 5, o = blockIdx.y, img = blockIdx.z;
  const int a0 = (blockIdx.x / g.tiles_x) * UC_H, b0 = (blockIdx.x % g.tiles_x) * UC_W;
  const int h = g.h, w = g.w, hw = h * w;
  const __amdgpu_buffer_rsrc_t zr = TG_BUF_RSRC(g.z + img * g.z_ns, (unsigned)(9 * g.cout) * hw * 4u);
  const __amdgpu_buffer_rsrc_t yr = TG_BUF_RSRC(g.y + img * g.y_ns, (unsigned)g.cout * hw * 16u);

  // row rr = tap * UC_ZH + ra of the staged planes: its offset in z, the row index clamped to the map
  auto z_row = [&](int rr) {
    const int tap = rr / UC_ZH;
    int a = a0 - 1 + (rr - tap * UC_ZH);
    a = a < 0 ? 0 : (a > h - 1 ? h - 1 : a);
    return (tap * g.cout + o) * hw + a * w;
  };
  const int bc = b0 + col < w ? b0 + col : w - 1;
  float zv[ZROUNDS];
#pragma unroll
  for (int it = 0; it < ZROUNDS; ++it) {                                      // the tile's own columns: every load in flight
    const int rr = rgrp + 8 * it;
    zv[it] = buf_ld<float>(zr, rr < ZROWS ? (unsigned)(z_row(rr) + bc) * 4u : BUF_OOB);
  }
#pragma unroll
  for (int it = 0; it < ZROUNDS; ++it) zs[(rgrp + 8 * it) * UC_ZW + 1 + col] = zv[it];
  for (int i = tid; i < 2 * ZROWS; i += 256) {                                // the halo columns
    const int rr = i >> 1, side = i & 1;
    const int b = side ? (b0 + UC_W < w ? b0 + UC_W : w - 1) : (b0 > 0 ? b0 - 1 : 0);
    zs[rr * UC_ZW + side * (UC_ZW - 1)] = buf_ld<float>(zr, (unsigned)(z_row(rr) + b) * 4u);
  }
  __syncthreads();

  // along x: hx[ky][row][X] = sum over kx of inside(X + kx - 1) * up2_x(z[ky, kx][row])[X + kx - 1], X = 2 b and 2 b + 1
  const bool first_col = b0 + col < 1, last_col = b0 + col >= w - 1;
#pragma unroll
  for (int it = 0; it < HROUNDS; ++it) {
    const int rw = rgrp + 8 * it, rd = rw < HROWS ? rw : HROWS - 1, ky = rd / UC_ZH;
    const float* z0 = zs + (2 * ky * UC_ZH + rd) * UC_ZW + 1 + col;           // (ky * 3) * UC_ZH + ra, ra = rd - ky * UC_ZH
    const float *z1 = z0 + UC_ZH * UC_ZW, *z2 = z1 + UC_ZH * UC_ZW;
    const float z0m = z0[-1], z0c = z0[0], z1m = z1[-1], z1c = z1[0], z1p = z1[1], z2c = z2[0], z2p = z2[1];
    f32x2 r;
    r[0] = (first_col ? 0.f : near_c(z0c, z0m)) + near_c(z1m, z1c) + near_c(z2p, z2c);      // columns 2b-1, 2b, 2b+1
    r[1] = near_c(z0m, z0c) + near_c(z1p, z1c) + (last_col ? 0.f : near_c(z2c, z2p));       // columns 2b, 2b+1, 2b+2
    *reinterpret_cast<f32x2*>(hx + rw * 2 * UC_W + 2 * col) = r;
  }
  __syncthreads();

  // along y, bias, activation: low row al -> output rows 2 al and 2 al + 1, four consecutive columns per thread
  const int al = tid >> 4, x4 = (tid & 15) * 4, ag = a0 + al, xo = 2 * b0 + x4;
  const float bv = buf_ld<float>(TG_BUF_RSRC(g.bias, g.bias ? (unsigned)g.cout * 4u : 0u), (unsigned)o * 4u);
  constexpr int ROW = 2 * UC_W / 4, KY = UC_ZH * ROW;                         // in float4
  const f32x4* h0 = reinterpret_cast<const f32x4*>(hx) + (1 + al) * ROW + (tid & 15);
  const f32x4 h0m = h0[-ROW], h0c = h0[0], h1m = h0[KY - ROW], h1c = h0[KY], h1p = h0[KY + ROW], h2c = h0[2 * KY],
              h2p = h0[2 * KY + ROW];
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 s0 = (ag < 1 ? zero : near_c(h0c, h0m)) + near_c(h1m, h1c) + near_c(h2p, h2c) + bv;   // rows 2a-1, 2a, 2a+1
  f32x4 s1 = near_c(h0m, h0c) + near_c(h1p, h1c) + (ag >= h - 1 ? zero : near_c(h2c, h2p)) + bv;
#pragma unroll
  for (int j = 0; j < 4; ++j) { s0[j] = apply_act(s0[j], g.act); s1[j] = apply_act(s1[j], g.act); }
  const unsigned row = (unsigned)((o * 2 * h + 2 * ag) * 2 * w);
  if constexpr (VEC) {
    const bool in = ag < h && xo < 2 * w;
    buf_st(s0, yr, in ? (row + xo) * 4u : BUF_OOB);
    buf_st(s1, yr, in ? (row + 2 * w + xo) * 4u : BUF_OOB);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool in = ag < h && xo + j < 2 * w;
      buf_st(s0[j], yr, in ? (row + xo + j) * 4u : BUF_OOB);
      buf_st(s1[j], yr, in ? (row + 2 * w + xo + j) * 4u : BUF_OOB);
    }
  }
}

static bool upconv_shape_ok(int cin, int cout) { return (cin == 64 || cin == 128 || cin == 256) && cout * 2 == cin; }
static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace tg

using namespace tg;

extern "C" size_t tg_upconv_packed_floats(int cin, int cout) {
  return upconv_shape_ok(cin, cout) ? (size_t)9 * cout * cin : 0;
}

extern "C" int tg_upconv_pack(const float* w, float* a_packed, int cin, int cout, int ocb, tg_stream_t stream) {
  TG_REQUIRE(w && a_packed, TG_E_ARG, "upconv_pack: null pointer");
  TG_REQUIRE(upconv_shape_ok(cin, cout) && (ocb == 0 || ocb == 32 || ocb == 64), TG_E_ARG,
             "upconv_pack: cin=%d cout=%d ocb=%d (cin 64 | 128 | 256, cout = cin / 2, ocb 0 | 32 | 64)", cin, cout, ocb);
  hipLaunchKernelGGL(upconv_pack_kernel, dim3(cdiv(9 * cout * cin, 256)), dim3(256), 0, (hipStream_t)stream, w, a_packed,
                     cin, cout, ocb);
  return check_launch("upconv_pack");
}

// what both launches check: the shape, and that one image's z and y stay below the 2 GiB a buffer record holds
static int upconv_args_ok(const char* who, int n, int cin, int cout, int h, int w) {
  TG_REQUIRE(upconv_shape_ok(cin, cout), TG_E_ARG, "%s: cin=%d cout=%d (cin 64 | 128 | 256, cout = cin / 2)", who, cin, cout);
  TG_REQUIRE(n > 0 && h > 0 && w > 0 && n <= 65535 && (long long)9 * cout * h * w * 4 < (1ll << 31), TG_E_ARG,
             "%s: n=%d h=%d w=%d", who, n, h, w);
  return TG_OK;
}

extern "C" int tg_upconv_tap_gemm(const float* x, int64_t x_nstride, const float* a_packed, float* z, int64_t z_nstride,
                                  int n, int cin, int cout, int h, int w, tg_stream_t stream) {
  TG_REQUIRE(x && a_packed && z, TG_E_ARG, "upconv_tap_gemm: null pointer");
  if (int rc = upconv_args_ok("upconv_tap_gemm", n, cin, cout, h, w)) return rc;
  TG_REQUIRE(aligned16(a_packed), TG_E_ARG, "upconv_tap_gemm: a_packed is not 16-byte aligned");
  const int hw = h * w, m = 9 * cout;
  TG_REQUIRE_NSTRIDE("upconv_tap_gemm", "x", x, x_nstride, n, (int64_t)cin * hw);
  TG_REQUIRE_NSTRIDE("upconv_tap_gemm", "z", z, z_nstride, n, (int64_t)m * hw);
  const UpGemmArgs g{x, a_packed, z, x_nstride, z_nstride, cin, m, hw};
  const dim3 grid(cdiv(hw, UG_PX), m / UG_M, n);
  const bool vec = hw % 4 == 0 && aligned16(x) && aligned16(z) && (n == 1 || (x_nstride % 4 == 0 && z_nstride % 4 == 0));
  if (vec) hipLaunchKernelGGL(upconv_tap_gemm_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, g);
  else hipLaunchKernelGGL(upconv_tap_gemm_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, g);
  return check_launch("upconv_tap_gemm");
}

extern "C" int tg_upconv_combine(const float* z, int64_t z_nstride, const float* bias, float* y, int64_t y_nstride, int n,
                                 int cout, int h, int w, int act, tg_stream_t stream) {
  TG_REQUIRE(z && y, TG_E_ARG, "upconv_combine: null pointer");
  if (int rc = upconv_args_ok("upconv_combine", n, 2 * cout, cout, h, w)) return rc;
  TG_REQUIRE(act >= TG_ACT_NONE && act <= TG_ACT_TANH24, TG_E_ARG, "upconv_combine: act=%d", act);
  TG_REQUIRE_NSTRIDE("upconv_combine", "z", z, z_nstride, n, (int64_t)9 * cout * h * w);
  TG_REQUIRE_NSTRIDE("upconv_combine", "y", y, y_nstride, n, (int64_t)cout * 4 * h * w);
  const int tiles_x = cdiv(w, UC_W);
  const UpCombineArgs g{z, bias, y, z_nstride, y_nstride, cout, h, w, act, tiles_x};
  const dim3 grid(tiles_x * cdiv(h, UC_H), cout, n);
  const bool vec = w % 2 == 0 && aligned16(y) && (n == 1 || y_nstride % 4 == 0);
  if (vec) hipLaunchKernelGGL(upconv_combine_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, g);
  else hipLaunchKernelGGL(upconv_combine_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, g);
  return check_launch("upconv_combine");
}

extern "C" int tg_upconv3x3_fwd(const float* x, int64_t x_nstride, const float* a_packed, const float* bias, float* z,
                                int64_t z_nstride, float* y, int64_t y_nstride, int n, int cin, int cout, int h, int w,
                                int act, tg_stream_t stream) {
  // what the combine would refuse is refused before the GEMM is launched
  TG_REQUIRE(x && a_packed && z && y && act >= TG_ACT_NONE && act <= TG_ACT_TANH24, TG_E_ARG,
             "upconv3x3_fwd: null pointer or act=%d", act);
  if (int rc = upconv_args_ok("upconv3x3_fwd", n, cin, cout, h, w)) return rc;
  TG_REQUIRE_NSTRIDE("upconv3x3_fwd", "y", y, y_nstride, n, (int64_t)cout * 4 * h * w);
  if (int rc = tg_upconv_tap_gemm(x, x_nstride, a_packed, z, z_nstride, n, cin, cout, h, w, stream)) return rc;
  return tg_upconv_combine(z, z_nstride, bias, y, y_nstride, n, cout, h, w, act, stream);
}

// TG_UPCONV, read once per process: 0 never, 1 wherever the kernels support the shape, unset the measured rule.
// With TG_CONV_WINO=1 the plan keeps the up-sampling folded into the Winograd staging (tests/test_hip_wino_fused.py).
extern "C" int tg_upconv_prefers(int n, int cin, int cout, int h, int w) {
  static const int env = [] { const char* e = getenv("TG_UPCONV"); return e && *e ? atoi(e) : -1; }();
  static const int wino = [] { const char* e = getenv("TG_CONV_WINO"); return e && *e ? atoi(e) : -1; }();
  if (env == 0 || wino == 1 || n <= 0 || h <= 0 || w <= 0 || !upconv_shape_ok(cin, cout)) return 0;
  if ((long long)9 * cout * h * w * 4 >= (1ll << 31) || n > 65535) return 0;
  if (env == 1) return 1;
  // The measured rule (EXPERIMENTS.md, "Up-sampling readers at the low resolution"): all three readers at the source maps
  // of a 134x320 frame, in every batched flow pass of 2 .. 8 frame pairs (-35 / -23 / -23 us at 8 pairs against the
  // up-sampling launch + Winograd conv).  Smaller maps were not measured, and the one-pair pass of the frame plan stays
  // as it is: decoder2.0 is a split-K pair there, and the tests' small plans keep the composed launches bit for bit.
  const int min_map = cin == 256 ? 16 * 40 : cin == 128 ? 32 * 80 : 64 * 160;
  return n >= 2 && h * w >= min_map ? 1 : 0;
}
