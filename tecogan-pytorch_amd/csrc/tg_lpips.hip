// LPIPS v0.1 (net='alex', model='net-lin', spatial=False) for gfx950:
// codes/metrics/LPIPS/models/networks_basic.py:25-99, pretrained_networks.py:57-95.
//
// Backbone = torchvision alexnet().features[0:12], taps relu1..relu5:
//   conv1 Conv2d(3,64,k11,s4,p2)+ReLU   -> lpips_conv_kernel<11,4,true>  (uint8 HWC in, ScalingLayer via LUT)
//   MaxPool2d(3,2)                       -> maxpool3s2_kernel
//   conv2 Conv2d(64,192,k5,p2)+ReLU      -> lpips_conv_kernel<5,1,false>
//   MaxPool2d(3,2)                       -> maxpool3s2_kernel
//   conv3..5 Conv2d 3x3 p1 + ReLU        -> tg_conv3x3_fwd (tg_conv3x3_mfma.hip)
// Head, per layer: normalize_tensor of both maps, squared difference, 1x1 lin weights, spatial mean
//   -> lpips_head_kernel (partials per workgroup) + lpips_head_final_kernel (fixed-order sum).
//
// lpips_conv_kernel is an fp32-MFMA implicit GEMM
//     D[oc][p] = sum_k Wt[k][oc] * X[k][p],   k = (ci*KS + ky)*KS + kx  (torch's weight order),
// p = (image, oy, ox).  Workgroup: 64 output channels x 128 pixels, 4 waves of 32 oc x 64 px, each
// wave two v_mfma_f32_32x32x2_f32 accumulators (A = weights: lane -> oc, B = patch: lane -> pixel).
// K streams through LDS in chunks of 32 (register-staged: chunk c+1 is loaded from global while chunk
// c is multiplied).  Every output is one k-ordered fma chain over its own image's pixels, so a
// result never depends on where the image sits in the batch or how frames are chunked.
#include "tg_common.h"

namespace tg {
namespace {

constexpr int LP_BM = 64;           // output channels per workgroup
constexpr int LP_BN = 128;          // output pixels per workgroup
constexpr int LP_BK = 32;           // K per LDS chunk
constexpr int LP_AS = LP_BM + 32;   // LDS row strides: rows kk and kk+1 (the two lane halves) 32 banks apart
constexpr int LP_BS = LP_BN + 32;
constexpr int LP_HEAD_THREADS = 256;

struct LpConvArgs {
  const void* x0;       // images [0, n0)
  const void* x1;       // images [n0, n) (may equal x0's continuation)
  const float* lut;     // U8: (256, 3) fp32 normalised value of byte v in channel c
  const float* wt;      // (K, cout): weights transposed, K = cin*KS*KS
  const float* bias;    // (cout)
  float* y;             // (n, cout, oh, ow)
  int n0, n, cin, h, w, cout, oh, ow, pad, K;
};

template <int KS, int S, bool U8>
__global__ __launch_bounds__(256) void lpips_conv_kernel(LpConvArgs a) {
  __shared__ float As[LP_BK * LP_AS];
  __shared__ float Bs[LP_BK * LP_BS];
  __shared__ float lut_s[U8 ? 768 : 1];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1;
  const int oc0 = blockIdx.y * LP_BM;
  const int ohw = a.oh * a.ow;
  const long long P = (long long)a.n * ohw;
  const long long p0 = (long long)blockIdx.x * LP_BN;

  if (U8) {
    for (int i = tid; i < 768; i += 256) lut_s[i] = a.lut[i];
  }

  // this thread's B column (fixed over K): pixel p0 + (tid & 127), k rows (tid >> 7) + 2 i
  const int bcol = tid & (LP_BN - 1);
  const int krow0 = tid >> 7;
  const long long p = p0 + bcol;
  const bool pvalid = p < P;
  int iy0 = 0, ix0 = 0;
  const uint8_t* img8 = nullptr;
  const float* img32 = nullptr;
  if (pvalid) {
    const int img = (int)(p / ohw);
    const int r = (int)(p - (long long)img * ohw);
    const int oy = r / a.ow, ox = r - (r / a.ow) * a.ow;
    iy0 = oy * S - a.pad;
    ix0 = ox * S - a.pad;
    const bool first = img < a.n0;
    const long long idx = first ? img : img - a.n0;
    if (U8)
      img8 = (const uint8_t*)(first ? a.x0 : a.x1) + idx * a.h * a.w * 3;
    else
      img32 = (const float*)(first ? a.x0 : a.x1) + idx * a.cin * a.h * a.w;
  }
  if (U8) __syncthreads();   // LUT visible before the first gather

  constexpr int NA = LP_BK * LP_BM / 256;   // 8 weight values per thread and chunk
  constexpr int NB = LP_BK * LP_BN / 256;   // 16 patch values per thread and chunk
  float ra[NA], rb[NB];

  auto load = [&](int k0) {
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int e = tid + 256 * i;
      const int m = e & (LP_BM - 1), kk = e >> 6;
      const int k = k0 + kk, oc = oc0 + m;
      ra[i] = (k < a.K && oc < a.cout) ? a.wt[(long long)k * a.cout + oc] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int k = k0 + krow0 + 2 * i;
      float v = 0.f;
      if (pvalid && k < a.K) {
        const int ci = k / (KS * KS);
        const int t = k - ci * (KS * KS);
        const int ky = t / KS, kx = t - (t / KS) * KS;
        const int iy = iy0 + ky, ix = ix0 + kx;
        if (iy >= 0 && iy < a.h && ix >= 0 && ix < a.w) {   // zero padding of the normalised input
          if (U8)
            v = lut_s[(int)img8[((long long)iy * a.w + ix) * 3 + ci] * 3 + ci];
          else
            v = img32[((long long)ci * a.h + iy) * a.w + ix];
        }
      }
      rb[i] = v;
    }
  };

  f32x16 acc[2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

  const int nchunk = cdiv(a.K, LP_BK);
  load(0);
  for (int c = 0; c < nchunk; ++c) {
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int e = tid + 256 * i;
      As[(e >> 6) * LP_AS + (e & (LP_BM - 1))] = ra[i];
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) Bs[(krow0 + 2 * i) * LP_BS + bcol] = rb[i];
    __syncthreads();
    if (c + 1 < nchunk) load((c + 1) * LP_BK);   // in flight during this chunk's MFMAs
    const int half = lane >> 5, l32 = lane & 31;
#pragma unroll
    for (int s = 0; s < LP_BK / 2; ++s) {
      const int kk = 2 * s + half;
      const float av = As[kk * LP_AS + wm * 32 + l32];
      const float b0 = Bs[kk * LP_BS + wn * 64 + l32];
      const float b1 = Bs[kk * LP_BS + wn * 64 + 32 + l32];
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b0, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b1, acc[1], 0, 0, 0);
    }
    __syncthreads();
  }

  // epilogue: C/D row (oc) = (r & 3) + 8 (r >> 2) + 4 (lane >> 5), column (pixel) = lane & 31
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const long long q = p0 + wn * 64 + j * 32 + (lane & 31);
    if (q >= P) continue;
    const int img = (int)(q / ohw);
    const int pix = (int)(q - (long long)img * ohw);
    float* yb = a.y + (long long)img * a.cout * ohw + pix;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int oc = oc0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      if (oc < a.cout) {
        const float v = acc[j][r] + a.bias[oc];
        yb[(long long)oc * ohw] = v > 0.f ? v : 0.f;
      }
    }
  }
}

// nn.MaxPool2d(3, 2), floor mode, no padding
__global__ __launch_bounds__(256) void maxpool3s2_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                         int nc, int h, int w, int oh, int ow) {
  const long long total = (long long)nc * oh * ow;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int ox = (int)(i % ow);
    const long long t = i / ow;
    const int oy = (int)(t % oh);
    const long long pl = t / oh;
    const float* s = x + (pl * h + 2 * oy) * w + 2 * ox;
    float m = s[0];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) m = fmaxf(m, s[dy * w + dx]);
    y[i] = m;
  }
}

// Head workgroup: 64 pixels (lane) x 4 channel groups (wave).  Blocks per frame are a function of the map size only
// (never of the batch), so each frame's partials -- and their fixed-order sum -- are the same wherever the frame sits.
constexpr int LP_HEAD_PIX = 64;
constexpr int LP_HEAD_GROUPS = LP_HEAD_THREADS / LP_HEAD_PIX;
inline int lpips_head_blocks(int h, int w) { return cdiv(h * w, LP_HEAD_PIX); }

// Per pixel: n0 = sqrt(sum_c a^2), n1 = sqrt(sum_c b^2), d = sum_c lin[c] (a/(n0+eps) - b/(n1+eps))^2 in fp32 (the
// reference's op order; each wave sums the channels g, g+4, ... and the four group sums are added in group order).
// The block's 64 values of d are summed in fp64 by a fixed tree into part[frame][block].
__global__ __launch_bounds__(LP_HEAD_THREADS) void lpips_head_kernel(const float* __restrict__ ft,
                                                                     const float* __restrict__ fp,
                                                                     const float* __restrict__ lin, int c, int hw,
                                                                     double* __restrict__ part) {
  __shared__ float sq[2][LP_HEAD_GROUPS][LP_HEAD_PIX];
  __shared__ float dd[LP_HEAD_GROUPS][LP_HEAD_PIX];
  __shared__ double red[LP_HEAD_PIX];
  const int f = blockIdx.y, nb = gridDim.x;
  const int lane = threadIdx.x % LP_HEAD_PIX, g = threadIdx.x / LP_HEAD_PIX;
  const int p = blockIdx.x * LP_HEAD_PIX + lane;
  const bool valid = p < hw;
  const float* a = ft + (long long)f * c * hw + p;
  const float* b = fp + (long long)f * c * hw + p;
  float s0 = 0.f, s1 = 0.f;
  if (valid) {
    for (int ch = g; ch < c; ch += LP_HEAD_GROUPS) {
      const float va = a[(long long)ch * hw], vb = b[(long long)ch * hw];
      s0 = fmaf(va, va, s0);
      s1 = fmaf(vb, vb, s1);
    }
  }
  sq[0][g][lane] = s0;
  sq[1][g][lane] = s1;
  __syncthreads();
  float t0 = sq[0][0][lane], t1 = sq[1][0][lane];
  for (int i = 1; i < LP_HEAD_GROUPS; ++i) { t0 += sq[0][i][lane]; t1 += sq[1][i][lane]; }
  const float d0 = sqrtf(t0) + 1e-10f, d1 = sqrtf(t1) + 1e-10f;
  float d = 0.f;
  if (valid) {
    for (int ch = g; ch < c; ch += LP_HEAD_GROUPS) {
      const float df = a[(long long)ch * hw] / d0 - b[(long long)ch * hw] / d1;
      d = fmaf(lin[ch], df * df, d);
    }
  }
  dd[g][lane] = d;
  __syncthreads();
  if (g == 0) {
    float v = dd[0][lane];
    for (int i = 1; i < LP_HEAD_GROUPS; ++i) v += dd[i][lane];
    red[lane] = (double)v;
  }
  __syncthreads();
  for (int s = LP_HEAD_PIX / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[(long long)f * nb + blockIdx.x] = red[0];
}

// res[f*5 + layer] = (sum of the frame's partials in block order) / hw; with total: also
// total[f] = res[f*5+0] + ... + res[f*5+4] in that order (val += res[l], networks_basic.py:86-88).
__global__ __launch_bounds__(64) void lpips_head_final_kernel(const double* __restrict__ part, int nb, int frames,
                                                              double inv_hw, float* __restrict__ res, int layer,
                                                              float* __restrict__ total) {
  const int f = blockIdx.x * 64 + threadIdx.x;
  if (f >= frames) return;
  double s = 0.0;
  for (int i = 0; i < nb; ++i) s += part[(long long)f * nb + i];
  const float v = (float)(s * inv_hw);
  res[f * 5 + layer] = v;
  if (total) {
    float t = res[f * 5 + 0];
    for (int l = 1; l < 5; ++l) t += (l == layer ? v : res[f * 5 + l]);
    total[f] = t;
  }
}

}  // namespace
}  // namespace tg

using namespace tg;

extern "C" int tg_lpips_conv_fwd(const void* x0, const void* x1, int n0, const float* lut, const float* wt,
                                 const float* bias, float* y, int n, int cin, int h, int w, int cout, int ks,
                                 int stride, int pad, tg_stream_t stream) {
  TG_REQUIRE(x0 && wt && bias && y, TG_E_ARG, "lpips_conv: null pointer");
  TG_REQUIRE(n > 0 && n0 >= 0 && n0 <= n && (n0 == n || x1), TG_E_ARG, "lpips_conv: n=%d n0=%d x1=%p", n, n0, x1);
  const bool u8 = lut != nullptr;
  TG_REQUIRE((ks == 11 && stride == 4 && u8 && cin == 3) || (ks == 5 && stride == 1 && !u8), TG_E_SHAPE,
             "lpips_conv: supported forms are k11/s4 on uint8 HWC with a LUT (cin 3) and k5/s1 on fp32 NCHW; "
             "got k%d s%d lut=%d cin=%d", ks, stride, (int)u8, cin);
  TG_REQUIRE(cin > 0 && cout > 0 && pad >= 0 && h + 2 * pad >= ks && w + 2 * pad >= ks, TG_E_SHAPE,
             "lpips_conv: cin=%d cout=%d h=%d w=%d k%d p%d", cin, cout, h, w, ks, pad);
  const int oh = (h + 2 * pad - ks) / stride + 1, ow = (w + 2 * pad - ks) / stride + 1;
  TG_REQUIRE((long long)n * cout * oh * ow < (1ll << 31) && (long long)n * cin * h * w < (1ll << 31), TG_E_SHAPE,
             "lpips_conv: batch too large (n=%d)", n);
  LpConvArgs a{};
  a.x0 = x0; a.x1 = x1 ? x1 : x0; a.lut = lut; a.wt = wt; a.bias = bias; a.y = y;
  a.n0 = x1 ? n0 : n; a.n = n; a.cin = cin; a.h = h; a.w = w; a.cout = cout; a.oh = oh; a.ow = ow;
  a.pad = pad; a.K = cin * ks * ks;
  const long long P = (long long)n * oh * ow;
  dim3 grid((unsigned)((P + LP_BN - 1) / LP_BN), (unsigned)cdiv(cout, LP_BM));
  if (u8)
    hipLaunchKernelGGL((lpips_conv_kernel<11, 4, true>), grid, dim3(256), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL((lpips_conv_kernel<5, 1, false>), grid, dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("lpips_conv");
}

extern "C" int tg_maxpool3s2_fwd(const float* x, float* y, int nc, int h, int w, tg_stream_t stream) {
  TG_REQUIRE(x && y, TG_E_ARG, "maxpool3s2: null pointer");
  TG_REQUIRE(nc > 0 && h >= 3 && w >= 3, TG_E_SHAPE, "maxpool3s2: nc=%d h=%d w=%d", nc, h, w);
  const int oh = (h - 3) / 2 + 1, ow = (w - 3) / 2 + 1;
  const long long total = (long long)nc * oh * ow;
  long long blocks = (total + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(maxpool3s2_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, y, nc, h, w,
                     oh, ow);
  return check_launch("maxpool3s2");
}

extern "C" int64_t tg_lpips_head_workspace_bytes(int frames, int h, int w) {
  if (frames <= 0 || h <= 0 || w <= 0) return -1;
  return (int64_t)frames * lpips_head_blocks(h, w) * (int64_t)sizeof(double);
}

extern "C" int tg_lpips_head(const float* feat_true, const float* feat_pred, const float* lin, int frames, int c,
                             int h, int w, void* ws, float* res, int layer, float* total, tg_stream_t stream) {
  TG_REQUIRE(feat_true && feat_pred && lin && ws && res, TG_E_ARG, "lpips_head: null pointer");
  TG_REQUIRE(frames > 0 && c > 0 && h > 0 && w > 0, TG_E_SHAPE, "lpips_head: frames=%d c=%d h=%d w=%d", frames, c,
             h, w);
  TG_REQUIRE(layer >= 0 && layer < 5 && (!total || layer == 4), TG_E_ARG,
             "lpips_head: layer=%d (0..4; the total is written with the last layer)", layer);
  TG_REQUIRE(frames <= 65535 && (long long)h * w < (1ll << 31), TG_E_SHAPE, "lpips_head: frames=%d h=%d w=%d",
             frames, h, w);
  const int nb = lpips_head_blocks(h, w);
  hipLaunchKernelGGL(lpips_head_kernel, dim3(nb, frames), dim3(LP_HEAD_THREADS), 0, (hipStream_t)stream, feat_true,
                     feat_pred, lin, c, h * w, (double*)ws);
  int rc = check_launch("lpips_head");
  if (rc != TG_OK) return rc;
  hipLaunchKernelGGL(lpips_head_final_kernel, dim3(cdiv(frames, 64)), dim3(64), 0, (hipStream_t)stream,
                     (const double*)ws, nb, frames, 1.0 / ((double)h * w), res, layer, total);
  return check_launch("lpips_head_final");
}
