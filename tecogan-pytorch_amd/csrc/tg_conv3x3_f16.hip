// fp16 inference body of SRNet: 3x3 convolutions on the f16 matrix cores with fp32 accumulation.
//
//   conv3x3_f16_kernel<false>  Conv2d(64, 64, 3, 1, 1): fp16 channels-last in, fp16 channels-last out,
//                              fp32 bias, optional ReLU, optional fp16 residual; ONE rounding, at the store
//   conv3x3_f16_kernel<true>   ConvTranspose2d(64, 64, 3, 2, 1, output_padding 1): fp16 channels-last in,
//                              fp32 NCHW out (unrounded), the layout the fp32 HR stage reads
//   pack_input_f16_kernel      two fp32 NCHW sources -> one fp16 channels-last tensor of 64 channels (zero padded)
//   pack_weights_f16_kernel    fp32 OIHW / IOHW -> fp16 in the order the A operand of the MFMA wants
//
// Implicit GEMM, D[cout][pixel] = sum_k W[cout][k] X[k][pixel] with k = tap * 64 + cin (K = 576 = 18 steps of 32) on
// v_mfma_f32_16x16x32_f16.  The WEIGHTS are the A operand and the pixels the B operand, so a lane's four accumulator
// registers are four consecutive output channels of one pixel (C/D map: column = lane & 15, row = 4 * (lane >> 4) + reg):
// the channels-last store is 8 bytes per lane and 16-channel tile.  The transposed convolution is the same loop: its
// nine taps fall into the four output parities (1, 2, 2 and 4 taps), each with an accumulator set of its own.
//
// One workgroup = 4 waves = a tile of 8 rows x 32 pixels, a wave = two rows (four 16-pixel groups x four 16-channel
// tiles: one weight fragment from LDS serves four MFMAs); the transposed form: 4 rows, one per wave.  The packed weights (72 KB) and the tile with its halo (fp16 channels-last, 144-byte pixel stride: 128 + 16
// so that the 16 pixels of a ds_read_b128 do not share banks) live in LDS; a workgroup loads the weights once and
// walks over tiles with a grid stride.  No workgroup waits for another one.
#include "tg_common.h"
#include "tg_launch.h"

namespace tg {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

constexpr int HC = 64;                         // channels (cin = cout = 64; fewer are zero padded by the packers)
constexpr int HKS = 18;                        // K steps of 32: 9 taps x 2 channel halves
constexpr int HW_HALVES = HKS * 4 * 64 * 8;    // packed weights: [K step][16-channel tile][lane][8]
constexpr int HW_BYTES = HW_HALVES * 2;        // 73728
constexpr int HPIX = 144;                      // LDS bytes per pixel
constexpr int HTC = 32;                        // tile columns (two 16-pixel groups)

template <bool CONVT> struct f16_geo {
  static constexpr int OFF = CONVT ? 0 : 1;                      // halo above / left of the tile
  static constexpr int RW = CONVT ? 1 : 2;                       // rows per wave (the transposed form holds 4 accumulator sets)
  static constexpr int TR = 4 * RW;                              // tile rows (4 waves)
  static constexpr int NG = 2 * RW;                              // 16-pixel groups per wave
  static constexpr int LH = TR + 1 + OFF, LW = HTC + 1 + OFF;    // (one row / column below / right in both forms)
  static constexpr int NCLS = CONVT ? 4 : 1;                     // accumulator sets (output parities)
  static constexpr int LDS_BYTES = HW_BYTES + LH * LW * HPIX;
};

template <bool CONVT>
__global__ __launch_bounds__(256) void conv3x3_f16_kernel(const _Float16* __restrict__ x, const _Float16* __restrict__ wp,
                                                          const float* __restrict__ bias, const _Float16* res,
                                                          _Float16* yh, float* __restrict__ yf, int64_t yf_ns,
                                                          int n, int h, int w, int relu) {
  using G = f16_geo<CONVT>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* const wl = smem;
  unsigned char* const tl = smem + HW_BYTES;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, p = lane & 15, q = lane >> 4;
  const int tcols = cdiv(w, HTC), trows = cdiv(h, G::TR);
  const int ntile = n * trows * tcols;
  // A tile's halo image travels global -> registers -> LDS.  All of a thread's loads are issued back to back (one
  // memory round trip per tile, not one per 16 bytes), and the NEXT tile's loads are issued before this tile's MFMAs,
  // so a workgroup that walks over several tiles waits for memory once.
  constexpr int TOT = G::LH * G::LW * 8;               // 16-byte pieces of the halo image
  constexpr int NIT = (TOT + 255) / 256;
  uint4 stage[NIT];
  auto fetch = [&](int tile) {
    const int img = tile / (trows * tcols);
    const int y0 = ((tile / tcols) % trows) * G::TR, x0 = (tile % tcols) * HTC;
    const _Float16* const xi = x + (int64_t)img * h * w * HC;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int idx = tid + it * 256;
      const int pix = idx >> 3, ch = idx & 7;
      const int ly = pix / G::LW, lx = pix - ly * G::LW;
      const int gy = y0 + ly - G::OFF, gx = x0 + lx - G::OFF;
      stage[it] = make_uint4(0u, 0u, 0u, 0u);          // zero padding
      if (idx < TOT && gy >= 0 && gy < h && gx >= 0 && gx < w)
        stage[it] = *reinterpret_cast<const uint4*>(xi + ((int64_t)gy * w + gx) * HC + ch * 8);
    }
  };
  if ((int)blockIdx.x < ntile) fetch(blockIdx.x);        // (in flight together with the weights)
  {
    const uint4* src = reinterpret_cast<const uint4*>(wp);
    uint4* dst = reinterpret_cast<uint4*>(wl);
#pragma unroll
    for (int i = 0; i < HW_BYTES / 16 / 256; ++i) dst[tid + i * 256] = src[tid + i * 256];
  }
  for (int tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const int img = tile / (trows * tcols);
    const int tr = (tile / tcols) % trows, tc = tile % tcols;
    const int y0 = tr * G::TR, x0 = tc * HTC;
    __syncthreads();                             // the previous tile's reads are done
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int idx = tid + it * 256;
      if (idx < TOT) *reinterpret_cast<uint4*>(tl + (idx >> 3) * HPIX + (idx & 7) * 16) = stage[it];
    }
    __syncthreads();
    if (tile + (int)gridDim.x < ntile) fetch(tile + gridDim.x);
    f32x4 acc[G::NCLS][G::NG][4];
#pragma unroll
    for (int c = 0; c < G::NCLS; ++c)
#pragma unroll
      for (int g = 0; g < G::NG; ++g)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) acc[c][g][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    // K step ks = tap * 2 + channel half.  Conv2d: input (y + ky - 1, x + kx - 1).  ConvTranspose2d, written per input
    // site i: output row 2i (parity 0) takes ky = 1 from row i; output row 2i + 1 (parity 1) takes ky = 0 from row i + 1
    // and ky = 2 from row i; columns alike.  The fragments of step ks + 1 are requested before the MFMAs of step ks:
    // with one wave per SIMD nothing else hides the LDS latency.
    f16x8 fa[2][4], fb[2][G::NG];
    auto frags = [&](int ks, f16x8 (&a)[4], f16x8 (&b)[G::NG]) {
      const int t = ks >> 1, hf = ks & 1, ky = t / 3, kx = t % 3;
      const int dy = CONVT ? (ky == 0 ? 1 : 0) : ky, dx = CONVT ? (kx == 0 ? 1 : 0) : kx;
#pragma unroll
      for (int g = 0; g < G::NG; ++g)
        b[g] = *reinterpret_cast<const f16x8*>(tl + ((wv * G::RW + (g >> 1) + dy) * G::LW + (g & 1) * 16 + p + dx) * HPIX +
                                               hf * 64 + q * 16);
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
        a[ct] = *reinterpret_cast<const f16x8*>(wl + ((ks * 4 + ct) * 64 + lane) * 16);
    };
    frags(0, fa[0], fb[0]);
#pragma unroll
    for (int ks = 0; ks < HKS; ++ks) {
      if (ks + 1 < HKS) frags(ks + 1, fa[(ks + 1) & 1], fb[(ks + 1) & 1]);
      const int ky = (ks >> 1) / 3, kx = (ks >> 1) % 3;
      const int cls = CONVT ? ((ky != 1 ? 2 : 0) + (kx != 1 ? 1 : 0)) : 0;
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int g = 0; g < G::NG; ++g)
          acc[cls][g][ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[ks & 1][ct], fb[ks & 1][g], acc[cls][g][ct], 0, 0, 0);
    }
    // epilogue: lane = pixel p of each group, channels ct * 16 + 4 q + (0..3)
    {
#pragma unroll
      for (int g = 0; g < G::NG; ++g) {
        const int gy = y0 + wv * G::RW + (g >> 1), gx = x0 + (g & 1) * 16 + p;
        if (gy >= h || gx >= w) continue;
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
          const int c0 = ct * 16 + q * 4;
          const float4 bv = *reinterpret_cast<const float4*>(bias + c0);
          const float bb[4] = {bv.x, bv.y, bv.z, bv.w};
          if constexpr (!CONVT) {
            const int64_t o = (((int64_t)img * h + gy) * w + gx) * HC + c0;
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              v[r] = acc[0][g][ct][r] + bb[r];
              if (relu) v[r] = v[r] > 0.f ? v[r] : 0.f;
            }
            if (res) {
              const f16x4 rv = *reinterpret_cast<const f16x4*>(res + o);
#pragma unroll
              for (int r = 0; r < 4; ++r) v[r] += (float)rv[r];
            }
            f16x4 hv;
#pragma unroll
            for (int r = 0; r < 4; ++r) hv[r] = (_Float16)v[r];          // round to nearest even, once
            *reinterpret_cast<f16x4*>(yh + o) = hv;
          } else {
            const int oh = 2 * h, ow = 2 * w;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              float* const plane = yf + (int64_t)img * yf_ns + (int64_t)(c0 + r) * oh * ow;
#pragma unroll
              for (int py = 0; py < 2; ++py) {
                float2 o2;
                o2.x = acc[py * 2 + 0][g][ct][r] + bb[r];
                o2.y = acc[py * 2 + 1][g][ct][r] + bb[r];
                if (relu) { o2.x = o2.x > 0.f ? o2.x : 0.f; o2.y = o2.y > 0.f ? o2.y : 0.f; }
                *reinterpret_cast<float2*>(plane + (int64_t)(2 * gy + py) * ow + 2 * gx) = o2;
              }
            }
          }
        }
      }
    }
  }
}

// one thread per (pixel, chunk of 8 channels; blockIdx.y): eight coalesced plane reads in flight, one 16-byte store.
// Channels come from two NCHW sources (c1 + c2 <= 64), the rest is zero.
__global__ __launch_bounds__(256) void pack_input_f16_kernel(const float* __restrict__ x1, int64_t x1_ns, int c1,
                                                             const float* __restrict__ x2, int64_t x2_ns, int c2,
                                                             _Float16* __restrict__ y, int n, int64_t hw) {
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= (int64_t)n * hw) return;
  const int ch = blockIdx.y;
  const int img = (int)(id / hw);
  const int64_t px = id - (int64_t)img * hw;
  const float* const s1 = x1 + (int64_t)img * x1_ns + px;
  const float* const s2 = x2 ? x2 + (int64_t)img * x2_ns + px : s1;
  float f[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = ch * 8 + j;                          // (block-uniform: the selects below are scalar)
    const float* const src = c < c1 ? s1 + (int64_t)c * hw : (c < c1 + c2 ? s2 + (int64_t)(c - c1) * hw : s1);
    f[j] = *src;                                       // always a valid address; padding channels are zeroed below
  }
  f16x8 v;
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = (ch * 8 + j < c1 + c2) ? (_Float16)f[j] : (_Float16)0.f;   // round to nearest even
  *reinterpret_cast<f16x8*>(y + id * HC + ch * 8) = v;
}

// out[((ks * 4 + ct) * 64 + lane) * 8 + j] = W[cout = 16 ct + (lane & 15)][tap = ks / 2][cin = 32 (ks & 1) + 8 (lane >> 4) + j]
// from OIHW (Conv2d) or IOHW (ConvTranspose2d, no flip: the kernel walks the taps in the transposed sense itself)
__global__ __launch_bounds__(256) void pack_weights_f16_kernel(const float* __restrict__ wsrc, _Float16* __restrict__ out,
                                                               int cin, int cout, int transposed) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= HW_HALVES) return;
  const int j = idx & 7, lane = (idx >> 3) & 63, ct = (idx >> 9) & 3, ks = idx >> 11;
  const int co = ct * 16 + (lane & 15), tap = ks >> 1, ci = (ks & 1) * 32 + (lane >> 4) * 8 + j;
  float v = 0.f;
  if (ci < cin && co < cout)
    v = transposed ? wsrc[((int64_t)ci * cout + co) * 9 + tap] : wsrc[((int64_t)co * cin + ci) * 9 + tap];
  out[idx] = (_Float16)v;
}

template <bool CONVT>
static int launch_f16(const _Float16* x, const _Float16* wp, const float* bias, const _Float16* res, _Float16* yh,
                      float* yf, int64_t yf_ns, int n, int h, int w, int act, tg_stream_t st, const char* what) {
  if (const int rc = ensure_dynamic_lds<conv3x3_f16_kernel<CONVT>>(f16_geo<CONVT>::LDS_BYTES, what)) return rc;
  const int64_t ntile = (int64_t)n * cdiv(h, f16_geo<CONVT>::TR) * cdiv(w, HTC);
  const int grid = (int)(ntile < 256 ? ntile : 256);       // one workgroup per CU (LDS), grid stride over the tiles
  hipLaunchKernelGGL(conv3x3_f16_kernel<CONVT>, dim3(grid), dim3(256), f16_geo<CONVT>::LDS_BYTES, (hipStream_t)st,
                     x, wp, bias, res, yh, yf, yf_ns, n, h, w, act == TG_ACT_RELU ? 1 : 0);
  return check_launch(what);
}

static bool f16_shape_ok(int n, int cin, int cout, int h, int w) {
  return n >= 1 && cin == HC && cout == HC && h >= 1 && w >= 1 && (int64_t)n * h * w < ((int64_t)1 << 31) / 4;
}

}  // namespace tg

using namespace tg;

extern "C" int tg_conv3x3_f16_supported(int n, int cin, int cout, int h, int w) {
  return f16_shape_ok(n, cin, cout, h, w) ? 1 : 0;
}

extern "C" size_t tg_conv3x3_f16_packed_halves(int cin, int cout) {
  return (cin >= 1 && cin <= HC && cout >= 1 && cout <= HC) ? (size_t)HW_HALVES : 0;
}

extern "C" int64_t tg_conv3x3_f16_act_halves(int n, int h, int w) {
  return (n >= 1 && h >= 1 && w >= 1) ? (int64_t)n * h * w * HC : -1;
}

extern "C" int tg_conv3x3_f16_pack_weights(const float* w, int cin, int cout, int transposed, uint16_t* out,
                                           tg_stream_t stream) {
  TG_REQUIRE(w && out, TG_E_ARG, "conv3x3_f16_pack_weights: null pointer");
  TG_REQUIRE(cin >= 1 && cin <= HC && cout >= 1 && cout <= HC, TG_E_SHAPE,
             "conv3x3_f16_pack_weights: cin=%d cout=%d (1..64 each)", cin, cout);
  hipLaunchKernelGGL(pack_weights_f16_kernel, dim3(HW_HALVES / 256), dim3(256), 0, (hipStream_t)stream, w,
                     reinterpret_cast<_Float16*>(out), cin, cout, transposed ? 1 : 0);
  return check_launch("conv3x3_f16_pack_weights");
}

extern "C" int tg_conv3x3_f16_pack_input(const float* x1, int64_t x1_nstride, int c1, const float* x2,
                                         int64_t x2_nstride, int c2, uint16_t* y, int n, int h, int w,
                                         tg_stream_t stream) {
  TG_REQUIRE(x1 && y && (x2 || c2 == 0), TG_E_ARG, "conv3x3_f16_pack_input: null pointer");
  TG_REQUIRE((reinterpret_cast<uintptr_t>(y) & 15) == 0, TG_E_ARG, "conv3x3_f16_pack_input: y must be 16-byte aligned");
  TG_REQUIRE(c1 >= 1 && c2 >= 0 && c1 + c2 <= HC && f16_shape_ok(n, HC, HC, h, w), TG_E_SHAPE,
             "conv3x3_f16_pack_input: n=%d c1=%d c2=%d h=%d w=%d (c1 + c2 <= 64)", n, c1, c2, h, w);
  const int64_t hw = (int64_t)h * w, tot = (int64_t)n * hw;
  TG_REQUIRE_NSTRIDE("conv3x3_f16_pack_input", "x1", x1, x1_nstride, n, c1 * hw);
  TG_REQUIRE_NSTRIDE("conv3x3_f16_pack_input", "x2", c2 ? x2 : nullptr, x2_nstride, n, c2 * hw);
  hipLaunchKernelGGL(pack_input_f16_kernel, dim3((unsigned)((tot + 255) / 256), 8), dim3(256), 0, (hipStream_t)stream, x1,
                     x1_nstride, c1, x2, x2_nstride, c2, reinterpret_cast<_Float16*>(y), n, hw);
  return check_launch("conv3x3_f16_pack_input");
}

extern "C" int tg_conv3x3_f16_fwd(const uint16_t* x, const uint16_t* w_packed, const float* bias, const uint16_t* res,
                                  uint16_t* y, int n, int cin, int cout, int h, int w, int act, tg_stream_t stream) {
  TG_REQUIRE(x && w_packed && bias && y, TG_E_ARG, "conv3x3_f16_fwd: null pointer");
  TG_REQUIRE(y != x, TG_E_ARG, "conv3x3_f16_fwd: y may not alias x (it may alias res)");
  TG_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(w_packed) |
               reinterpret_cast<uintptr_t>(res) | reinterpret_cast<uintptr_t>(bias)) & 15) == 0, TG_E_ARG,
             "conv3x3_f16_fwd: pointers must be 16-byte aligned");
  TG_REQUIRE(act == TG_ACT_NONE || act == TG_ACT_RELU, TG_E_ARG, "conv3x3_f16_fwd: act %d (none | relu)", act);
  TG_REQUIRE(f16_shape_ok(n, cin, cout, h, w), TG_E_SHAPE, "conv3x3_f16_fwd: n=%d cin=%d cout=%d h=%d w=%d (64 -> 64)",
             n, cin, cout, h, w);
  return launch_f16<false>(reinterpret_cast<const _Float16*>(x), reinterpret_cast<const _Float16*>(w_packed), bias,
                           reinterpret_cast<const _Float16*>(res), reinterpret_cast<_Float16*>(y), nullptr, 0, n, h, w,
                           act, stream, "conv3x3_f16_fwd");
}

extern "C" int tg_convt3x3s2_f16_fwd(const uint16_t* x, const uint16_t* w_packed, const float* bias, float* y,
                                     int64_t y_nstride, int n, int cin, int cout, int h, int w, int act,
                                     tg_stream_t stream) {
  TG_REQUIRE(x && w_packed && bias && y, TG_E_ARG, "convt3x3s2_f16_fwd: null pointer");
  TG_REQUIRE(act == TG_ACT_NONE || act == TG_ACT_RELU, TG_E_ARG, "convt3x3s2_f16_fwd: act %d (none | relu)", act);
  TG_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(w_packed) | reinterpret_cast<uintptr_t>(bias)) & 15) == 0,
             TG_E_ARG, "convt3x3s2_f16_fwd: pointers must be 16-byte aligned");
  TG_REQUIRE((reinterpret_cast<uintptr_t>(y) & 7) == 0 && (y_nstride & 1) == 0, TG_E_ARG,
             "convt3x3s2_f16_fwd: y must be 8-byte aligned and y_nstride even");
  TG_REQUIRE(f16_shape_ok(n, cin, cout, h, w) && y_nstride >= (int64_t)cout * 4 * h * w, TG_E_SHAPE,
             "convt3x3s2_f16_fwd: n=%d cin=%d cout=%d h=%d w=%d (64 -> 64)", n, cin, cout, h, w);
  return launch_f16<true>(reinterpret_cast<const _Float16*>(x), reinterpret_cast<const _Float16*>(w_packed), bias,
                          nullptr, nullptr, y, y_nstride, n, h, w, act, stream, "convt3x3s2_f16_fwd");
}
