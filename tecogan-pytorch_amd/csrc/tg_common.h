// Shared helpers for libtecogan_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <stdlib.h>

#include "../../include/tecogan_hip.h"

// Switches read from the environment (TG_LAB_ENV: one kernel form forced where the launcher would choose by shape)
// exist only in lab builds (TG_LAB_BUILD=1 OUT=<dir> bash build.sh, which sets -DTG_LAB=1).  The one compile-time lab
// switch is WR_UASM=0 (tg_conv3x3_wino_res.hip: the cross-check form of the resident kernel's weight loads); the
// row chain's per-layer time stamps (tg_conv3x3_chain.hip) are compiled in by TG_LAB itself.  The ablation and A/B
// variants of rounds 1-6 are in EXPERIMENTS.md and in git history.  The shipped library reads exactly four variables,
// all documented in INTEGRATION.md: TG_CONV_WINO, TG_WINO_CHAIN, TG_WINO_RES and TG_UPCONV (kernel-form selection
// for A/B runs; every setting produces reference-parity results).  The Python mirror has switches of its own
// (TG_FNET_BATCH, TG_WINO_RES_CT, TG_CONV4_DIRECT, TECOGAN_COMM, TECOGAN_HIP_LIB): INTEGRATION.md.
#ifndef TG_LAB
#define TG_LAB 0
#endif
#if TG_LAB
#define TG_LAB_ENV(name, dflt) ([] { const char* e_ = getenv(name); return e_ ? atoi(e_) : (dflt); }())
#else
#define TG_LAB_ENV(name, dflt) (dflt)
#endif

namespace tg {

void set_error(const char* fmt, ...);

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: %s", what, hipGetErrorString(e));
    return TG_E_HIP;
  }
  return TG_OK;
}

#define TG_REQUIRE(cond, code, ...) \
  do {                              \
    if (!(cond)) {                  \
      tg::set_error(__VA_ARGS__);   \
      return (code);                \
    }                               \
  } while (0)

// The batch-stride contract of every entry that takes a `*_nstride` (KERNELS.md, "Buffer placement"): the images of one
// operand do not overlap, i.e. with n > 1 the stride of a non-null operand is at least the floats of one image.  A
// launcher indexes image b at b * nstride and nothing else, so a smaller stride silently computes on / over the
// neighbouring image.  TG_E_SHAPE, nothing is launched.
#define TG_REQUIRE_NSTRIDE(entry, name, ptr, ns, n, floats)                                                      \
  TG_REQUIRE(!(ptr) || (n) <= 1 || (long long)(ns) >= (long long)(floats), TG_E_SHAPE,                           \
             entry ": " name "_nstride=%lld is less than the %lld floats of one image", (long long)(ns), \
             (long long)(floats))
// ... of layer `i` of a launch that takes its strides per layer (the one-launch bodies)
#define TG_REQUIRE_LAYER_NSTRIDE(entry, i, name, ptr, ns, n, floats)                                             \
  TG_REQUIRE(!(ptr) || (n) <= 1 || (long long)(ns) >= (long long)(floats), TG_E_SHAPE,                           \
             entry ": layer %d: " name "_nstride=%lld is less than the %lld floats of one image", (int)(i),      \
             (long long)(ns), (long long)(floats))

// whether tg_convt3x3s2_z_fwd_form(form) runs as two launches (whole rounds of 4-row workgroups + a 2-row tail)
bool convt_z_split_rule(int n, int h, int w, int form);
// whether tg_convt3x3s2_z_wino_fwd(split) runs as two launches (whole rounds of resident workgroups + a remainder)
bool convt_z_wino_split_rule(int n, int h, int w, int split);

// split-K halves of tg_conv3x3_splitk_fwd (the plan accounts them as separate kernel classes)
int conv3x3_splitk_conv(const float* x, int64_t x_nstride, int c1, const float* x2,
                        int64_t x2_nstride, const float* w_packed, int ocb, int n, int cin,
                        int cout, int h, int w, int ksplit, float* partials, tg_stream_t stream);
int conv3x3_splitk_finalize(const float* partials, int ksplit, const float* bias, int act, int pool,
                            float* y, int n, int cout, int h, int w, tg_stream_t stream);

// rows of the image one conv3x3 workgroup covers (selects the kernel variant):
// 64-oc blocks use the 4-row / 2-tile-per-wave variant on big images and the
// 2-row variant (twice the workgroups) where tile quantisation dominates.
inline int conv3x3_rows_per_wg(int ocb, long long pixels) {
  if (ocb == 32) return 4;
  return pixels >= 200000 ? 4 : 2;
}

__host__ __device__ inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// 64-channel-group layers with at most half as many 2-row tiles as CUs run the in-workgroup
// K-split variant of the conv kernel (1-row tiles, two wave groups over alternating chunks).
bool conv3x3_uses_wg_ksplit(int n, int cin, int cout, int h, int w);
bool conv3x3_uses_oneshot(int n, int cin, int cout, int h, int w);
// Winograd F(2x2,3x3) form (tg_conv3x3_wino.hip); arguments as tg_conv3x3_wino_fwd, unchecked but for `fuse`
// (TG_WINO_POOL / TG_WINO_UP2 as in tg_conv3x3_wino_fused_fwd; conv3x3_wino_fuse_ok says which shapes take them)
bool conv3x3_wino_fuse_ok(int cin, int h, int w, int fuse);
bool conv3x3_wino_folds_up2(int n, int cin, int cout, int h, int w);     // the plan's (measured) rule for TG_WINO_UP2
int conv3x3_wino_launch(const float* x, int64_t x_ns, int c1, const float* x2, int64_t x2_ns, const float* u,
                        const float* bias, const float* res, int64_t res_ns, const float* mask,
                        int64_t mask_ns, float* y, int64_t y_ns, int n, int cin, int cout, int h, int w,
                        int act, tg_stream_t stream, int fuse = 0);

// several dependent Winograd layers in one launch (tg_conv3x3_wino.hip); err: int32 fault counter in
// device or pinned host memory, poll_limit < 0 injects a fault into every waiting workgroup
constexpr int TG_CHAIN_POLL_LIMIT_DEFAULT = 1 << 21;
int conv3x3_wino_chain_launch(const tg_wino_layer* layers, int n_layers, int n, int cout, int h, int w,
                              int32_t* flags, int32_t* err, unsigned epoch, int poll_limit, tg_stream_t stream);

// SRNet's conv_in + residual-block convs of one frame as ONE launch of persistent, LDS-resident workgroups
// (tg_conv3x3_wino_res.hip): supported shapes, workspace (exchange buffer + flags + 256 bytes), launch
bool conv3x3_wino_resident_ok(int n, int cout, int h, int w);
int64_t conv3x3_wino_resident_ws_bytes(int h, int w);
int conv3x3_wino_resident_launch(const tg_wino_layer* layers, int n_layers, int cout, int h, int w, void* ws,
                                 int32_t* err, unsigned base, int poll_limit, tg_stream_t stream,
                                 const tg_wres_convt* ct = nullptr);

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// ---- raw buffer access ----------------------------------------------------
// How the kernels address an operand in global memory (KERNELS.md, "Buffer access"): a 128-bit descriptor {base, record
// bytes} built once per operand from wave-uniform values, and a 32-bit per-lane BYTE offset checked against the record
// bytes by the hardware -- a load past them returns 0 and a store past them is dropped, which is how every kernel gets
// its zero padding, its channel padding and its masked lanes without a branch.  This section is the only place that
// spells out the gfx950 builtins (tests/test_buffer_access_cpu.py).
//
// Word 3 of the descriptor: DATA_FORMAT (bits 18:15) = 4, a 32-bit format -- the field must not be 0 (an invalid
// descriptor), the untyped buffer_load / buffer_store_dword* instructions do not otherwise read it.  All else is 0:
// no swizzle, no add-tid, and with stride 0 (word 1) a raw buffer, whose range check is `offset + size > record bytes`.
constexpr int BUF_RSRC_FLAGS = 0x00020000;
// A macro and not a function: through an inline function the row chain's two output descriptors came out with a dozen
// re-ordered scalar instructions and a few re-scheduled v_pk_add_f32 (EXPERIMENTS.md); the macro is the builtin call.
// ptr: any (const) object pointer, wave-uniform; bytes: the record length, below 2^31 (BUF_OOB).
#define TG_BUF_RSRC(ptr, bytes) \
  __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(static_cast<const void*>(ptr)), 0, (bytes), ::tg::BUF_RSRC_FLAGS)

// The offset of an element that does not exist.  Contract: every record length built here is below 2 GiB (one operand
// of one batch item; the launchers' shape checks keep tensors under that), so this offset -- and any offset that
// wrapped below zero, e.g. a channel that belongs to the other source tensor -- is out of range for EVERY descriptor:
// the load returns 0, the store is dropped.
constexpr unsigned BUF_OOB = 0x80000000u;

// Cache-policy (aux) bit sc1 of the buffer instructions on gfx940+: agent scope.  The access goes to / comes from the
// memory side of the cache hierarchy instead of this CU's L1 and this XCD's non-coherent L2 copy.  Mandatory on EVERY
// store of, and EVERY load of, data that another workgroup of the SAME launch produces or consumes: the chained
// Winograd launch (tg_conv3x3_wino.hip), the row chain (tg_conv3x3_chain.hip) and the resident launch's ring exchange
// (tg_conv3x3_wino_res.hip).  Data written by an earlier launch needs no bit (0): a kernel boundary makes it visible.
constexpr int BUF_SC1 = 16;

// T: a 4-, 8- or 16-byte trivially copyable type (float, f32x2, f32x4, u32x4, ...); voff: per-lane byte offset (VGPR),
// soff: wave-uniform byte offset (SGPR) added to it; AUX: 0 or BUF_SC1.
template <typename T, int AUX = 0>
__device__ __forceinline__ T buf_ld(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff = 0) {
  static_assert(__is_trivially_copyable(T) && (sizeof(T) == 4 || sizeof(T) == 8 || sizeof(T) == 16), "b32 / b64 / b128");
  if constexpr (sizeof(T) == 4) return __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b32(r, (int)voff, (int)soff, AUX));
  else if constexpr (sizeof(T) == 8) return __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b64(r, (int)voff, (int)soff, AUX));
  else return __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, AUX));
}
template <int AUX = 0, typename T>
__device__ __forceinline__ void buf_st(T v, __amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff = 0) {
  static_assert(__is_trivially_copyable(T) && (sizeof(T) == 4 || sizeof(T) == 8 || sizeof(T) == 16), "b32 / b64 / b128");
  if constexpr (sizeof(T) == 4) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, (int)voff, (int)soff, AUX);
  else if constexpr (sizeof(T) == 8) __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), r, (int)voff, (int)soff, AUX);
  else __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, (int)voff, (int)soff, AUX);
}

// input-channel chunk streamed through LDS per K-step group
constexpr int CK = 8;

__device__ __forceinline__ float apply_act(float v, int act) {
  switch (act) {
    case TG_ACT_RELU: return v > 0.f ? v : 0.f;
    case TG_ACT_LRELU02: return v >= 0.f ? v : v * 0.2f;
    case TG_ACT_TANH24: return tanhf(v) * 24.f;
    default: return v;
  }
}

// Negative-side slope of the piecewise-linear activations: x >= 0 ? x : x*slope
// (1 = identity, 0 = ReLU, 0.2 = LeakyReLU(0.2)); wave-uniform, branch free.
__device__ __forceinline__ float act_slope(int act) {
  return act == TG_ACT_RELU ? 0.f : (act == TG_ACT_LRELU02 ? 0.2f : 1.f);
}

inline float act_slope_host(int act) {
  return act == TG_ACT_RELU ? 0.f : (act == TG_ACT_LRELU02 ? 0.2f : 1.f);
}

// ---- shared sampling arithmetic (device) ---------------------------------
// BicubicUpsampler weights (net_utils.py:113-127), a = -0.75, fp32, evaluated
// exactly as cubic @ [1, s, s^2, s^3] with s = d/f.
__device__ __forceinline__ void bicubic_w(int d, int f, float k[4]) {
  const float a = -0.75f;
  float s = (float)d / (float)f;  // 1.0*d/f in double then fp32 in the reference; d/f exact for f in {2,4}
  float s2 = s * s, s3 = s2 * s;
  // rows of the Keys matrix times [1, s, s2, s3], left-to-right accumulation
  k[0] = ((0.f * 1.f + a * s) + (-2.f * a) * s2) + a * s3;
  k[1] = ((1.f * 1.f + 0.f * s) + (-(a + 3.f)) * s2) + (a + 2.f) * s3;
  k[2] = ((0.f * 1.f + (-a) * s) + (2.f * a + 3.f) * s2) + (-(a + 2.f)) * s3;
  k[3] = ((0.f * 1.f + 0.f * s) + a * s2) + (-a) * s3;
}

// F.interpolate(bilinear, align_corners=False), integer scale: source taps.
__device__ __forceinline__ void bilinear_src(int dst, int scale, int in_size,
                                             int& i0, int& i1, float& l0,
                                             float& l1) {
  float src = ((float)dst + 0.5f) * (1.0f / (float)scale) - 0.5f;
  src = src < 0.f ? 0.f : src;
  i0 = (int)floorf(src);
  i1 = i0 + 1 < in_size ? i0 + 1 : in_size - 1;
  l1 = src - (float)i0;
  l0 = 1.0f - l1;
}

// The four taps of bilinear_src blended along x, then along y: `l0 * a + l1 * b` of the up-sampling kernels with the
// multiply-add fusion written out (what -ffp-contract=on makes of that expression: the left product is fused, the
// right one rounded) and further contraction off, so that every call site -- the up-sampling kernels of tg_warp.hip
// and the x2 up-sampling folded into the Winograd conv's staging (tg_conv3x3_wino.hip) -- rounds alike, bit for bit.
__device__ __forceinline__ float bilinear_blend(float lx0, float lx1, float ly0, float ly1, float v00, float v01,
                                                float v10, float v11) {
#pragma clang fp contract(off)
  const float top = __builtin_fmaf(lx0, v00, lx1 * v01);
  const float bot = __builtin_fmaf(lx0, v10, lx1 * v11);
  return __builtin_fmaf(ly0, top, ly1 * bot);
}

// fp32 torch.linspace(-1, 1, n)[i] (ATen CPU: two fused multiply-adds)
// Branch- and select-free form (round 4: v_cndmask_b32 costs ~23 cycles per wave instruction on gfx950,
// tools/valu_lab.hip): with j = min(i, n-1-i) the second half is -fmaf(step, j, -1) -- round-to-nearest is
// sign symmetric, so that is fmaf(-step, j, 1) bit for bit (but for the sign of an exact zero, which the
// callers add 1 to) -- and the sign bit comes from the integer n/2 - 1 - i.
__device__ __forceinline__ float linspace_m1p1(int i, int n, float step) {
  const int mirror = n - 1 - i;
  const int j = i < mirror ? i : mirror;                                   // v_min_i32
  const unsigned flip = (unsigned)(n / 2 - 1 - i) & 0x80000000u;           // i >= n/2
  return __builtin_bit_cast(float, __builtin_bit_cast(unsigned, __builtin_fmaf(step, (float)j, -1.0f)) ^ flip);
}

// Sampling position of backward_warp along one axis (net_utils.py:62-78 +
// grid_sample align_corners=True, padding_mode='border').
__device__ __forceinline__ float warp_coord(int i, int n, float flow) {
  float step = 2.0f / (float)(n - 1);
  float half = (float)(n - 1) / 2.0f;
  float g = linspace_m1p1(i, n, step) + flow / half;
  float p = (g + 1.0f) * half;
  p = __builtin_fmaxf(p, 0.f);                       // clip_coordinates (v_max / v_min: no conditional moves)
  p = __builtin_fminf(p, (float)(n - 1));
  return p;
}

}  // namespace tg
