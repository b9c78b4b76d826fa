/*
 * tecogan_hip.h -- C ABI of libtecogan_hip.so (MI355X / gfx950 only).
 *
 * The upstream reference (skycrapers/TecoGAN-PyTorch) has NO native code and
 * therefore no FFI of its own: its hot path is Python calling stock ATen ops.
 * This header is the boundary a maintainer binds instead of those ATen calls;
 * each entry cites the reference call site it replaces (paths relative to the
 * upstream repo root).  INTEGRATION.md shows the ctypes stub.
 *
 * Conventions
 *   - all tensors are fp32, contiguous NCHW unless a batch stride is given;
 *     pointers are DEVICE pointers owned by the caller (PyTorch allocates);
 *     the library never retains them past the call and never allocates device memory
 *     (a frame plan owns one 64-byte pinned-host fault counter, see tg_frnet_plan_chain_status);
 *   - `*_nstride` = distance in floats between consecutive batch items, so a
 *     channel-slice of a larger buffer can be read / written in place (this is
 *     how every torch.cat on the path is folded away);
 *   - `stream` is a hipStream_t passed as void*; every call only enqueues
 *     kernels on it (no hidden synchronisation, hipGraph-capturable);
 *   - every entry returns 0 (TG_OK) or a negative TG_E_* code;
 *     tg_last_error_string() describes the last failure on this thread.
 *     No C++ exception crosses the boundary.
 *
 * What this header may contain
 *   tecogan-pytorch_amd/_lib.py derives the Python binding from this text (no C compiler is involved): an
 *   entry is callable from Python once it is declared here and the library is rebuilt.  The parser refuses,
 *   at import and by name, whatever is not one of these; it never skips or guesses:
 *   - comments of this form only, and the preprocessor lines below as they stand, plus
 *     `#define TG_NAME <integer or parenthesised product of integers>` on one line;
 *   - `enum { TG_NAME = integer, ... };` -- anonymous, every value written out;
 *   - `typedef void* NAME;` (a handle passed by value) and `typedef struct NAME NAME;` (opaque);
 *   - `typedef struct [tag] { fields } NAME;` whose fields are int, int32_t, int64_t, unsigned, uint32_t,
 *     uint64_t, size_t, float, double (several names may share one such declaration) or pointers, one per
 *     declaration: no arrays, bit-fields, nested structs or function pointers.  A struct the package
 *     constructs also gets its Python name in _lib.py;
 *   - prototypes `type tg_name(type name, ...);` or `(void)`: every parameter named; one-word scalar
 *     types from the list above by value; pointers and `type name[N]` arrays to those, to void, char,
 *     uint8_t, uint16_t, int16_t and to the types declared here, `const` where it belongs.  A `T*` parameter whose T
 *     is a struct with fields is type-checked as that struct; every other pointer is an untyped address.
 *     A struct must be declared above its first use.
 */
#ifndef TECOGAN_HIP_H
#define TECOGAN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* tg_stream_t;

enum {
  TG_OK = 0,
  TG_E_SHAPE = -1, /* unsupported / inconsistent shape */
  TG_E_ARG = -2,   /* null pointer, bad enum */
  TG_E_HIP = -3    /* HIP runtime error at launch */
};

/* fused epilogue activation of the conv kernels */
enum {
  TG_ACT_NONE = 0,
  TG_ACT_RELU = 1,    /* nn.ReLU                 tecogan_nets.py:96,113,121,125 */
  TG_ACT_LRELU02 = 2, /* nn.LeakyReLU(0.2)       tecogan_nets.py:24-64, 369   */
  TG_ACT_TANH24 = 3   /* torch.tanh(.) * 24      tecogan_nets.py:80           */
};

/* up-sampling flavour: get_upsampling_func, codes/utils/net_utils.py:85-97 */
enum {
  TG_UP_NONE = 0,
  TG_UP_BICUBIC = 1, /* BicubicUpsampler (BD), net_utils.py:101-156 */
  TG_UP_BILINEAR = 2 /* F.interpolate bilinear align_corners=False (BI), :86-89 */
};

/* ABI version, major * 100 + minor.  The major number changes whenever a struct declared here
 * changes size or an entry changes its signature (a host compiled against another major must not
 * call in: check tg_version() / 100 == TG_ABI_MAJOR after dlopen).
 *   1xx: round-1 ABI.   2xx (minor 1: + chained training launches, phased_masked): tg_layer_weights gained `u` (24 bytes, was 16);
 *   tg_frnet_plan_chain_error_index replaced by tg_frnet_plan_chain_status. */
#define TG_ABI_MAJOR 2
int tg_version(void);
const char* tg_last_error_string(void);
/* How this library was built (a static string): "lab=<0|1> wres_lab_bits=<n> flags=<hipcc flags of csrc/build.sh>
 * file_flags=<per-file TG_FILE_FLAGS>".  The in-tree library is lab=0 wres_lab_bits=0 by construction (build.sh
 * refuses EXTRA_FLAGS / TG_LAB for it, the sources #error on a lab switch without TG_LAB); tests/test_abi_cpu.py
 * asserts exactly that, so an ablation build can never pass for the product. */
const char* tg_build_info(void);

/* ------------------------------------------------------------------------
 * 3x3 stride-1 pad-1 convolution, fp32 MFMA implicit GEMM.
 * Replaces every nn.Conv2d(.,.,3,1,1) on the path:
 *   FNet tecogan_nets.py:23-65, SRNet conv_in :111-113, ResidualBlock :92-98,
 *   D conv_in :367-369.
 * Fused: channel-concat of two sources (torch.cat :71, :141), bias,
 * activation, residual add (`self.conv(x) + x` :98).
 *
 * Weights must be pre-packed with tg_conv3x3_pack (layout private to the
 * kernel: [oc-group][cin-chunk][tap][8 cin][ocb oc], zero padded).
 *   ocb: output channels per workgroup, 32 or 64 (use tg_conv3x3_pick_ocb).
 * ---------------------------------------------------------------------- */
int tg_conv3x3_pick_ocb(int cout);
size_t tg_conv3x3_packed_floats(int cin, int cout, int ocb);
/* w_oihw: (cout, cin, 3, 3) as nn.Conv2d.weight.  transposed=1: w is
 * (cin, cout, 3, 3) as nn.ConvTranspose2d.weight (used by tg_convt3x3s2_fwd).
 * transposed=2: data-gradient packing of a Conv2d weight: the op maps the conv's
 * cout -> cin, i.e. call with cin := conv.cout, cout := conv.cin and w the
 * ORIGINAL (conv.cout, conv.cin, 3, 3) tensor; taps are rotated by 180 degrees. */
int tg_conv3x3_pack(const float* w, float* w_packed, int cin, int cout, int ocb,
                    int transposed, tg_stream_t stream);

int tg_conv3x3_fwd(
    const float* x, int64_t x_nstride, int c1,   /* channels [0,c1) from x          */
    const float* x2, int64_t x2_nstride,         /* channels [c1,cin) from x2 (or NULL) */
    const float* w_packed, int ocb, const float* bias /* may be NULL */,
    const float* res, int64_t res_nstride,       /* optional residual, added after act */
    float* y, int64_t y_nstride,
    int n, int cin, int cout, int h, int w, int act, tg_stream_t stream);

/* conv3x3 with PHASE-RESTRICTED TAPS: the strided layers run through their space-to-depth
 * embeddings -- Conv2d(k4, s2, p1) of the discriminator blocks (tecogan_nets.py:322-340) is a 3x3
 * conv on space_to_depth(x, 2) with 4*ci input channels, its data gradient a 3x3 conv onto
 * 4*ci output channels, and the data gradient of ConvTranspose2d(k3, s2, p1, op1) (:119-126) a
 * 3x3 conv on space_to_depth(dY, 2).  In those embedded weights every sub-pixel phase
 * (py, px) owns only some tap rows / columns; the others are zeros.  This entry skips them:
 *   tapsel 1: the phase of the INPUT channel chunk ((channel / cphase): py = phase >> 1,
 *             px = phase & 1) selects the taps; tapsel 2: the phase of the OUTPUT block does;
 *   taps_phase0 / taps_phase1: tap set used by phase coordinate 0 / 1 along each axis,
 *             0 = {0,1,2}, 1 = {0,1}, 2 = {1,2}, 3 = {1}.
 * Results equal tg_conv3x3_fwd on the same (zero-padded) weights up to summation order. */
int tg_conv3x3_fwd_phased(const float* x, int64_t x_nstride, const float* w_packed, int ocb,
                          const float* bias, float* y, int64_t y_nstride, int n, int cin,
                          int cout, int h, int w, int act, int tapsel, int cphase,
                          int taps_phase0, int taps_phase1, tg_stream_t stream);
/* nn.Conv2d(ci, co, 4, 2, 1, bias=False) -- the discriminator blocks (tecogan_nets.py:322-340) -- taken directly
 * (K = 16 ci implicit GEMM on the fp32 matrix cores, no space-to-depth copy, no phase masks) and its data gradient
 * (the 4x4 / stride-2 transposed convolution; optionally multiplied by act'(act_y) of the layer below on the way
 * out: act_y (n, ci, h, w) the activation OUTPUT that was this conv's input, act = TG_ACT_RELU | TG_ACT_LRELU02).
 * x, dx: (n, ci, h, w); y, g: (n, co, h/2, w/2), contiguous.  Weights: tg_conv4x4s2_pack from OIHW (co, ci, 4, 4)
 * into two buffers of tg_conv4x4s2_packed_floats(ci, co) floats (either may be NULL).
 * tg_conv4x4s2_supported: ci, co multiples of 64, h even, w a multiple of 64 -- or the small maps of the deeper
 * blocks, w = 32 (h % 8 == 0) / w = 16 (h % 16 == 0): 32 pixels of the matrix tile are then 2 / 4 rows, the input
 * channels are split over several workgroups and a second launch adds the partial sums in a fixed order; such calls
 * need tg_conv4x4s2_workspace_floats(.., dgrad) floats of workspace (0: none, workspace may be NULL).  Other shapes
 * keep the embedded form (tg_conv3x3_fwd_phased on tg_space_to_depth(x, 2)), and so does the weight gradient.
 * Alignment (TG_E_ARG otherwise): tg_conv4x4s2_dgrad stores dx and reads act_y as pairs of pixels, both 8-byte aligned;
 * the calls that need a workspace, and the small-map dgrad with act_y, also run a 16-byte pass over y / dx, the
 * workspace and act_y: 16-byte aligned. */
int tg_conv4x4s2_supported(int n, int ci, int co, int h, int w);
size_t tg_conv4x4s2_packed_floats(int ci, int co);
int tg_conv4x4s2_pack(const float* w, float* w_fwd, float* w_dgrad, int ci, int co, tg_stream_t stream);
size_t tg_conv4x4s2_workspace_floats(int n, int ci, int co, int h, int w, int dgrad);
int tg_conv4x4s2_fwd(const float* x, const float* w_fwd, float* y, float* workspace, int n, int ci, int co, int h, int w,
                     tg_stream_t stream);
int tg_conv4x4s2_dgrad(const float* g, const float* w_dgrad, const float* act_y, int act, float* dx, float* workspace,
                       int n, int ci, int co, int h, int w, tg_stream_t stream);
/* STRIDE-2 3x3 conv on small frames: y(oy, ox) = act(sum_k w[k] x(2 oy - 1 + ky, 2 ox - 1 + kx) + bias),
 * zero outside x (n, cin, 2 h_out, 2 w_out) -- the data gradient of ConvTranspose2d(k3, s2, p1, op1)
 * (tecogan_nets.py:119-126) taken directly (K = 9 cin) instead of through the 4 cin-channel phased
 * embedding; w_packed = tg_conv3x3_pack(W as (cout = ci, cin = co), ocb 64).  relu_mask as in
 * tg_conv3x3_fwd_masked.  tg_conv3x3s2_supported: cin, cout <= 64 and <= 1024 one-row tiles. */
int tg_conv3x3s2_supported(int n, int cin, int cout, int h_out, int w_out);
int tg_conv3x3s2_fwd(const float* x, int64_t x_nstride, const float* w_packed, const float* bias,
                     const float* relu_mask, int64_t mask_nstride, float* y, int64_t y_nstride, int n,
                     int cin, int cout, int h_out, int w_out, int act, tg_stream_t stream);
/* the same with a ReLU-backward mask in the epilogue (see tg_conv3x3_fwd_masked): the data gradient
 * of a transposed conv delivers dZ of the ReLU layer below it directly (relu_mask may be NULL) */
int tg_conv3x3_fwd_phased_masked(const float* x, int64_t x_nstride, const float* w_packed, int ocb,
                                 const float* bias, const float* relu_mask, int64_t mask_nstride,
                                 float* y, int64_t y_nstride, int n, int cin, int cout, int h, int w,
                                 int act, int tapsel, int cphase, int taps_phase0, int taps_phase1,
                                 tg_stream_t stream);
/* The same launch with the channel chunks split over `ksplit` workgroup sets (deterministic: partial sums
 * [ksplit][n][cout][h][w] in `partials`, added in a fixed order by the finalize launch, which also applies
 * bias / act) -- for the critic's deeper blocks, whose 48-192 tiles cannot fill 256 CUs.
 * tg_conv3x3_phased_pick_ksplit returns the recommended factor (1 = use tg_conv3x3_fwd_phased). */
int tg_conv3x3_phased_pick_ksplit(int n, int cin, int cout, int h, int w, int ocb);
int tg_conv3x3_fwd_phased_splitk(const float* x, int64_t x_nstride, const float* w_packed, int ocb,
                                 const float* bias, float* y, int n, int cin, int cout, int h, int w,
                                 int act, int tapsel, int cphase, int taps_phase0, int taps_phase1,
                                 int ksplit, float* partials, tg_stream_t stream);
/* tg_conv3x3_fwd followed by a ReLU-backward mask in the same epilogue:
 *   y = relu_mask > 0 ? y : 0      (relu_mask: (n,cout,h,w) fp32, e.g. a ReLU layer's output)
 * Used by the training tape: the data-gradient conv of a layer (weights packed with
 * transposed = 2) then delivers dZ of the PRECEDING ReLU layer directly, without a separate
 * activation-backward pass (torch.autograd's threshold_backward). */
int tg_conv3x3_fwd_masked(const float* x, int64_t x_nstride, int c1, const float* x2,
                          int64_t x2_nstride, const float* w_packed, int ocb,
                          const float* bias, const float* res, int64_t res_nstride,
                          const float* relu_mask, int64_t mask_nstride, float* y,
                          int64_t y_nstride, int n, int cin, int cout, int h, int w, int act,
                          tg_stream_t stream);

/* The same convolution (nn.Conv2d(k3, s1, p1), tecogan_nets.py:85-100,116) in the Winograd
 * F(2x2, 3x3) form: 16 instead of 36 fp32 MFMA multiplies per 2x2 output tile.  All arithmetic is
 * fp32 (the transform matrices hold only 0, +-1, +-1/2); results equal tg_conv3x3_fwd up to fp32
 * summation order.  `u_packed` comes from tg_pack_conv3x3_wino (tg_conv3x3_wino_packed_floats(cin,
 * cout) floats; transposed = 0 for OIHW weights, 2 for the data gradient: channel roles swapped,
 * taps rotated by 180 degrees).  x2 / res / relu_mask as in tg_conv3x3_fwd / _masked (may be NULL). */
int64_t tg_conv3x3_wino_packed_floats(int cin, int cout);
/* 1 when the Winograd form is the faster one for this layer shape on an MI355X (at least 160 16-tile
 * workgroups, cout a multiple of 64, cin >= 16; or cout = 32, cin >= 32 and at least 2048 32-tile
 * workgroups: FNet's two full-resolution layers in a batched flow pass); the frame plan uses it to pick
 * the form of each layer whose tg_layer_weights.u is set. */
int tg_conv3x3_prefers_wino(int n, int cin, int cout, int h, int w);
int tg_pack_conv3x3_wino(const float* w, float* out, int cin, int cout, int transposed,
                         tg_stream_t stream);
int tg_conv3x3_wino_fwd(const float* x, int64_t x_nstride, int c1, const float* x2,
                        int64_t x2_nstride, const float* u_packed, const float* bias,
                        const float* res, int64_t res_nstride, const float* relu_mask,
                        int64_t mask_nstride, float* y, int64_t y_nstride, int n, int cin,
                        int cout, int h, int w, int act, tg_stream_t stream);
/* The same kernel with a neighbouring memory-bound layer folded in (single source, no residual, no mask); h, w are the
 * conv's own map size and must be even, results are BIT-IDENTICAL to the two separate launches:
 *   TG_WINO_POOL: y = MaxPool2d(2, 2)(act(conv(x))), y (n, cout, h/2, w/2) -- the max over the 2x2 output tile a lane
 *                 holds anyway; the full-resolution tensor is never written.
 *   TG_WINO_UP2:  y = act(conv(bilinear_x2(x))), x (n, cin, h/2, w/2) -- the input staging blends every element from its
 *                 <= 4 source values (tg_upsample_fwd's taps, weights and expression); the up-sampled tensor never exists.
 * The two flags are not combined.  Other shapes / combinations: TG_E_SHAPE / TG_E_ARG, nothing is launched. */
#define TG_WINO_POOL 1
#define TG_WINO_UP2 2
int tg_conv3x3_wino_fused_fwd(const float* x, int64_t x_nstride, const float* u_packed, const float* bias,
                              float* y, int64_t y_nstride, int n, int cin, int cout, int h, int w, int act,
                              int fuse, tg_stream_t stream);

/* y = act(conv3x3(bilinear_x2(x)) + bias) with the matrix work at the LOW resolution (tg_upconv.hip): FNet's three
 * readers of a decoder block's up-sampling (tecogan_nets.py:44-64).  Up-sampling acts per channel and a tap's channel
 * mix per pixel, so they commute: a tap GEMM z[img][tap][o][pixel] = sum_c W[o][c][tap] x[img][c][pixel] on the
 * (h, w) source map (a quarter of the direct form's multiplies, fp32 MFMA), then a streaming combine
 * y[o][Y][X] = act(bias[o] + sum over taps of inside(Y+ky-1, X+kx-1) * bilinear_x2(z[tap][o])[Y+ky-1][X+kx-1]).
 * Equal to tg_upsample_fwd + tg_conv3x3_fwd up to fp32 summation order; two launches give identical bits.
 *   x (n, cin, h, w) -> z (n, 9 cout, h, w) scratch -> y (n, cout, 2h, 2w); h, w: the SOURCE map.
 *   supported: cin 64 | 128 | 256 with cout = cin / 2, 9 cout h w below 2^29; anything else is TG_E_ARG.
 *   a_packed: tg_upconv_pack of the layer's weights, tg_upconv_packed_floats(cin, cout) floats (0: unsupported),
 *             16-byte aligned; ocb 0: w is OIHW (cout, cin, 3, 3), 32 | 64: w is tg_conv3x3_pack(transposed = 0) with that ocb.
 *   16-byte accesses run where the operands are 16-byte aligned with strides and map sizes that keep them so, else
 *   element by element: same results.
 * tg_upconv_prefers: 1 where the frame plan runs a reader this way (n images, SOURCE map h x w).  TG_UPCONV=0 never,
 * 1 wherever supported, unset the measured rule; always 0 with TG_CONV_WINO=1 (the up-sampling then rides in the
 * Winograd kernel's staging).  Whatever it says, the plan keeps a reader whose conv is a split-K pair
 * (tg_conv3x3_pick_ksplit > 1: conv + finalize), so that its launch counts per kind do not depend on the form. */
size_t tg_upconv_packed_floats(int cin, int cout);
int tg_upconv_pack(const float* w, float* a_packed, int cin, int cout, int ocb, tg_stream_t stream);
int tg_upconv_tap_gemm(const float* x, int64_t x_nstride, const float* a_packed, float* z, int64_t z_nstride,
                       int n, int cin, int cout, int h, int w, tg_stream_t stream);
int tg_upconv_combine(const float* z, int64_t z_nstride, const float* bias, float* y, int64_t y_nstride, int n,
                      int cout, int h, int w, int act, tg_stream_t stream);
int tg_upconv3x3_fwd(const float* x, int64_t x_nstride, const float* a_packed, const float* bias, float* z,
                     int64_t z_nstride, float* y, int64_t y_nstride, int n, int cin, int cout, int h, int w,
                     int act, tg_stream_t stream);
int tg_upconv_prefers(int n, int cin, int cout, int h, int w);

/* Several DEPENDENT 3x3 layers (layer i+1 reads what layer i writes: SRNet's conv_in and residual
 * blocks, tecogan_nets.py:108-116,141-143) in ONE launch.  Every separate launch of the Winograd
 * kernel pays ~10 us that nothing overlaps (launch, first loads, final stores); here the workgroups
 * of layer i+1 are dispatched behind those of layer i and start as soon as the 3x3 tile
 * neighbourhood they read has been written (per-tile flags, agent-scope loads / stores).  A
 * workgroup only waits for workgroups with a smaller block index; forward progress relies on the
 * dispatcher starting workgroups in block order (true of every CDNA part, not promised by HIP), so
 * the kernel is fail-safe: a poll limit turns a lost flag into a fault count instead of a hang.
 *   layers[i]: as tg_conv3x3_wino_fwd (x2 / bias / res may be NULL; res is added after the
 *              activation; y may alias res: in-place residual sum); cout <= 64 for every layer.
 *              Any 4-byte aligned base; with n > 1 every *_nstride is at least one image (TG_E_SHAPE).
 *              The float2 epilogue runs only while y and res of EVERY layer are 8-byte aligned with even
 *              strides (and w, h w even), else every layer stores element by element: same results.
 *   flags:     tg_conv3x3_wino_chain_flag_ints(n_layers, n, h, w) int32, caller owned, zeroed ONCE
 *              before the first call; its last 16 ints are a fault counter the caller MUST read
 *              after synchronising (non-zero: a workgroup gave up waiting -- never seen; the
 *              results are then undefined.  The frame plan does this for its own chain, see
 *              tg_frnet_plan_chain_status).
 *   epoch:     any non-zero value not used before with these flags (a frame counter).
 * Buffers may be reused along the chain only in the patterns of the reference's SRNet: a layer may
 * overwrite a tensor that the PREVIOUS layer read, or its own residual input. */
typedef struct {
  const float* x; const float* x2; const float* u_packed; const float* bias; const float* res;
  float* y;
  int64_t x_nstride, x2_nstride, res_nstride, y_nstride;
  int c1, cin, act;
} tg_wino_layer;
int64_t tg_conv3x3_wino_chain_flag_ints(int n_layers, int n, int h, int w);
int tg_conv3x3_wino_chain(const tg_wino_layer* layers, int n_layers, int n, int cout, int h, int w,
                          int32_t* flags, int epoch, tg_stream_t stream);

/* The same DEPENDENT layers of ONE frame (n = 1) on persistent, LDS-RESIDENT workgroups (round 4;
 * tg_conv3x3_wino_res.hip): one workgroup per CU owns an 8 x 24 pixel block of the frame for ALL the
 * layers; the 64-channel block (+ a one-pixel ring) of the current and of the next layer live in LDS,
 * and between two layers only the block's outermost pixels travel through an exchange buffer in
 * global memory (16 KB per workgroup instead of 11 MB written + 11 MB read per layer at 134x320).
 * Same arithmetic in the same order as tg_conv3x3_wino_fwd: BIT-IDENTICAL results.
 *   supported: n == 1, cout == 64, even h and w, ceil(h/8) * ceil(w/24) <= CUs - 8 (every workgroup must
 *              be resident at once: neighbours wait for each other).  134x320 -> 238 workgroups.
 *   layers:    as tg_conv3x3_wino_chain with the buffer pattern of the reference's SRNet made a
 *              REQUIREMENT: layers[i].x == layers[i-1].y, layers[i].res in {NULL, layers[i-1].x},
 *              cin == 64 for i > 0, bias non-NULL.  Only layers[0].x / x2 are read and only
 *              layers[n_layers-1].y is written: the intermediate tensors never reach memory.
 *              x / x2: any 4-byte aligned base; layers[n_layers-1].y: 8-byte aligned (TG_E_ARG), strides unused.
 *   workspace: tg_conv3x3_wino_resident_ws_bytes(h, w) bytes, 256-byte aligned, caller owned, zeroed ONCE
 *              before the first call; its last 256 bytes hold a fault counter (int32) the caller MUST
 *              read after synchronising (non-zero: a workgroup gave up waiting for a neighbour; the
 *              results are then undefined.  The frame plan does this for its own launch).
 *   epoch:     1, 2, 3, ... strictly increasing per call on one workspace. */
int tg_conv3x3_wino_resident_supported(int n, int cout, int h, int w);
int64_t tg_conv3x3_wino_resident_ws_bytes(int h, int w);
int tg_conv3x3_wino_resident(const tg_wino_layer* layers, int n_layers, int cout, int h, int w,
                             void* workspace, int epoch, tg_stream_t stream);
/* The launch's hand-over geometry, on the host (no device work): where workgroup `block` (row-major over
 * ceil(h/8) x ceil(w/24)) finds pixel `ring_pixel` of its one-pixel ring (0..25 the row above the block from its
 * top-left corner, 26..51 the row below, 52..59 the column to the left, 60..67 the column to the right).  The kernel
 * tabulates the same function once per launch.  Writes the block that owns the pixel, the slot (0..63: top row,
 * bottom row 24.., left column 48.., right column 56..) under which that block publishes it, and the pixel's float
 * offset inside a channel of the LDS block (row stride 28); returns 1, or 0 for a pixel outside the image (owner and
 * slot are then -1), TG_E_SHAPE for odd or non-positive h / w, TG_E_ARG for a bad block, ring pixel or pointer. */
int tg_conv3x3_wino_resident_ring_item(int h, int w, int block, int ring_pixel, int* owner_block, int* owner_slot,
                                       int* lds_offset);
/* The same launch with SRNet's FIRST up-sampling layer (nn.ConvTranspose2d(64, 64, 3, 2, 1, output_padding=1) + ReLU,
 * tecogan_nets.py:119-126) as its tail: after the last conv layer's ring exchange every workgroup applies the
 * transposed convolution to its resident 8x24 block (+1 ring pixel right / below) and writes convt->y
 * (64, 2h, 2w); layers[n_layers-1].y is then NOT written.  Direct fp32 MFMA products (no Winograd): the result
 * equals tg_convt3x3s2_fwd on the same input up to the summation order (about 1e-6 relative).
 * u_packed: tg_conv3x3_wino_resident_ct_pack of the layer's (cin 64, cout 64, 3, 3) weights
 * (tg_conv3x3_wino_resident_ct_floats() floats).  convt == NULL: tg_conv3x3_wino_resident. */
typedef struct tg_wres_convt {
  const float* u_packed;
  const float* bias;
  float* y;
  int act;
} tg_wres_convt;
size_t tg_conv3x3_wino_resident_ct_floats(void);
int tg_conv3x3_wino_resident_ct_pack(const float* w_iohw, float* out, tg_stream_t stream);
int tg_conv3x3_wino_resident_ct(const tg_wino_layer* layers, int n_layers, int cout, int h, int w,
                                void* workspace, int epoch, const tg_wres_convt* convt, tg_stream_t stream);

/* Dependent 3x3 layers of SMALL frames (the training unroll: 2 x 32 x 32 / 2 x 64 x 64 LR pixels per
 * frame, tecogan_nets.py:174-225) in ONE launch: one persistent workgroup per (image row, 32-pixel
 * segment[, 32-channel half]) walks all the layers and exchanges halo rows with its neighbours
 * through agent-scope memory + per-tile flags (tg_conv3x3_chain.hip).  Direct fp32-MFMA form.  The
 * launcher picks the workgroups per tile from the shape (tg_conv3x3_chain_supported) and the weights must be
 * packed for that choice -- pack_layout 64: tg_conv3x3_pack with ocb = 64 (transposed = 0 forward, 2 data
 * gradient) for 1 or 2 workgroups per tile (32 x 32 x 2 MFMAs); pack_layout 16: tg_conv3x3_pack16
 * (tg_conv3x3_pack16_floats() floats per layer) for 4 workgroups per tile (16 x 16 x 4 MFMAs, the
 * smallest frames); a mismatch is TG_E_ARG.
 *   layers[i]: x (+ x2: channels [c1, cin)) -> y = relu_mask > 0 ? act(conv + bias) + res : 0;
 *              cin, cout <= 64; bias / res / relu_mask / x2 may be NULL; buffers may be reused along the
 *              chain in SRNet's patterns only (ping-pong, in-place residual sum).  Any 4-byte aligned base;
 *              with n > 1 every *_nstride is at least one image (TG_E_SHAPE).
 *   flags:     tg_conv3x3_chain_flag_ints(n_layers, n, h, w) int32, caller owned, zeroed ONCE.
 *   err:       int32 fault counter, device OR pinned host memory (the kernel adds with system scope):
 *              a workgroup that exhausts poll_limit polls (~32 cycles each; < 0: at once = fault
 *              injection) counts a fault and carries on -- the launch always ends; a non-zero count
 *              after synchronisation means the output is undefined and the caller must fall back to
 *              one launch per layer.
 *   epoch:     non-zero, different from the previous call on these flags.
 * Every workgroup must be resident at once: tg_conv3x3_chain_supported returns 0 when the grid would
 * exceed half of what the device holds (the call then fails with TG_E_SHAPE), else the number of
 * workgroups per tile it will use (1, 2 or 4). */
typedef struct {
  const float* x; const float* x2; const float* w_packed; const float* bias; const float* res;
  const float* relu_mask;
  float* y;
  int64_t x_nstride, x2_nstride, res_nstride, mask_nstride, y_nstride;
  int c1, cin, cout, act;
} tg_chain_layer;
int64_t tg_conv3x3_chain_flag_ints(int n_layers, int n, int h, int w);
int tg_conv3x3_chain_supported(int n, int h, int w, int cmax);
size_t tg_conv3x3_pack16_floats(void);
int tg_conv3x3_pack16(const float* w, float* w_packed, int cin, int cout, int transposed, tg_stream_t stream);
/* All the layers of a chain packed by one launch.  Item: source weights (O, i_total, 3, 3), of which the
 * input-channel slice [i_off, i_off + I) is used; transposed 0: the layer (cin = I, cout = O), 2: its data
 * gradient (cin = O, cout = I); out: tg_conv3x3_chain_packed_floats(pack_layout, cin) floats, in the layout
 * of tg_conv3x3_pack16 (16) / tg_conv3x3_pack with ocb 64 (64). */
typedef struct tg_pack_item {
  const float* w;
  float* out;
  int cin, cout, transposed, i_total, i_off;
} tg_pack_item;
size_t tg_conv3x3_chain_packed_floats(int pack_layout, int cin);
int tg_conv3x3_chain_pack(const tg_pack_item* items, int n_items, int pack_layout, tg_stream_t stream);
int tg_conv3x3_chain(const tg_chain_layer* layers, int n_layers, int n, int h, int w, int pack_layout,
                     int32_t* flags, int32_t* err, uint32_t epoch, int poll_limit, tg_stream_t stream);
/* SRNet's conv_in + nb residual blocks on one training frame (tecogan_nets.py:108-116, :141-143) and
 * the matching reverse sweep, each as one tg_conv3x3_chain launch.  acts / dz: 1 + 2*nb tensors
 * (n, nf, h, w) back to back, acts[0] = conv_in's output, acts[1+2b] / acts[2+2b] = block b's inner
 * activation / output; dz[i] = gradient w.r.t. the pre-activation of layer i -- dz[2nb], the gradient of
 * the body's output, is the INPUT the caller fills before the call -- d_tran = gradient w.r.t. the
 * warped-frame input channels (n, c_tran, h, w).
 * layers[i] / dgrad[i]: forward / data-gradient packs of layer i (dgrad[0]: conv_in restricted to
 * input channels [c_lr, c_lr + c_tran), bias unused). */
typedef struct { const float* w; const float* b; } tg_packed_layer;
int tg_srnet_body_fwd(const tg_packed_layer* layers, int pack_layout, int nb, const float* lr, int c_lr,
                      const float* tran, int c_tran, float* acts, int n, int nf, int h, int w, int32_t* flags,
                      int32_t* err, uint32_t epoch, int poll_limit, tg_stream_t stream);
int tg_srnet_body_bwd(const tg_packed_layer* dgrad, int pack_layout, int nb, const float* acts, float* dz,
                      float* d_tran, int c_tran, int n, int nf, int h, int w, int32_t* flags, int32_t* err,
                      uint32_t epoch, int poll_limit, tg_stream_t stream);

/* Weight / bias gradients of the chained body's layers for ALL unrolled frames in one launch each.
 * dz_bases[f] / act_bases[f]: the dz / acts blocks of frame f (tg_srnet_body_bwd / _fwd),
 * layer_stride = n_per_frame * c * h * w.
 *   tg_wgrad3x3_body: grads[L - 1] (+)= dW of layer L = 1 .. nlayers (= 2 * nb; conv_in, whose input has
 *     other channel counts, goes through tg_wgrad3x3_multi); workspace: tg_wgrad3x3_body_workspace_floats.
 *   tg_bias_grad_body: dbs[L] += db of layer L = 0 .. nlayers - 1 (= 1 + 2 * nb layers, conv_in included). */
size_t tg_wgrad3x3_body_workspace_floats(int nframes, int n_per_frame, int nlayers, int c, int h, int w);
int tg_wgrad3x3_body(const float* const* dz_bases, const float* const* act_bases, int nframes, int64_t layer_stride, int nlayers, float* const* grads, float* workspace,
                     int n_per_frame, int c, int h, int w, int accumulate, tg_stream_t stream);
/* ... and their bias gradients in the same pass: dbs[L - 1] (c floats) (+)= sum of dZ of layer L = 1..nlayers. */
int tg_wgrad3x3_body_bias(const float* const* dz_bases, const float* const* act_bases, int nframes,
                          int64_t layer_stride, int nlayers, float* const* grads, float* const* dbs,
                          float* workspace, int n_per_frame, int c, int h, int w, int accumulate,
                          tg_stream_t stream);
int tg_bias_grad_body(const float* const* dz_bases, int nframes,
                      int64_t layer_stride, int nlayers, float* const* dbs, int n_per_frame, int c, int hw,
                      tg_stream_t stream);

/* Split-K variant for layers whose output tile count cannot fill the GPU (FNet's
 * low-resolution many-channel middle, tecogan_nets.py:37-60): `ksplit` groups of
 * input channels are reduced by different workgroups into `partials`
 * (ksplit * n*cout*h*w floats, caller owned), then a finalize pass adds them in a
 * fixed order (bit-reproducible) and applies bias + activation and, when
 * pool != 0, the following nn.MaxPool2d(2,2) (y is then (n,cout,h/2,w/2)).
 * tg_conv3x3_pick_ksplit returns the recommended factor (1 = use tg_conv3x3_fwd). */
int tg_conv3x3_pick_ksplit(int n, int cin, int cout, int h, int w);
int tg_conv3x3_splitk_fwd(const float* x, int64_t x_nstride, int c1, const float* x2,
                          int64_t x2_nstride, const float* w_packed, int ocb,
                          const float* bias, float* y, int n, int cin, int cout, int h,
                          int w, int act, int ksplit, float* partials, int pool,
                          tg_stream_t stream);

/* ------------------------------------------------------------------------
 * ConvTranspose2d(cin, cout, 3, stride 2, padding 1, output_padding 1) + bias
 * + activation, as 4 sub-pixel phase GEMMs (no zero MACs), fp32 MFMA.
 * Replaces SRNet.conv_up, tecogan_nets.py:119-126.   y is (n, cout, 2h, 2w).
 * Weights packed with tg_conv3x3_pack(..., ocb=64, transposed=1).
 * ---------------------------------------------------------------------- */
int tg_convt3x3s2_fwd(const float* x, int64_t x_nstride, const float* w_packed,
                      const float* bias, float* y, int64_t y_nstride, int n,
                      int cin, int cout, int h, int w, int act,
                      tg_stream_t stream);
/* The HR stage without the 64-channel HR tensor (inference; SRNet.forward tecogan_nets.py:119-131,
 * 145): the LAST ConvTranspose2d + ReLU, run in "Z mode", contracts its output over the channels
 * with conv_out's weights while the values are still in the MFMA accumulators and stores the
 * 9*cz tap planes  z[tap*cz + o] = sum_oc Wout[o][oc][tap] * relu(convT(x)[oc] + b[oc])
 * (cz = out_nc <= 3; z is (n, 32, 2h, 2w), the first 9*cz planes written); tg_convout_tail
 * shift-adds them (zero padding of conv_out), adds conv_out's bias and upsample_func(lr_curr),
 * and optionally emits the uint8 HWC frame.  Same result as tg_convt3x3s2_fwd +
 * tg_conv3x3_small_fwd(_u8) up to summation order; 74 MB written + read instead of 176 MB.
 * tg_convt_pack_wz packs conv_out's OIHW weights (cz, nf, 3, 3) into the 2048-float operand. */
int tg_convt_pack_wz(const float* w_out_oihw, float* wz, int cz, int nf, tg_stream_t stream);
int tg_convt3x3s2_z_fwd(const float* x, int64_t x_nstride, const float* w_packed,
                        const float* bias, const float* wz, int cz, float* z,
                        int64_t z_nstride, int n, int cin, int cout, int h, int w, int act,
                        tg_stream_t stream);
/* The same with the kernel form chosen by the caller (any other value: TG_E_ARG):
 *  -1 = the library's rule (what tg_convt3x3s2_z_fwd does: 0 or 3 by shape),
 *   0 = tiled in one launch (one workgroup per 4-row x 32-pixel tile, 2-row tiles on small maps; weights staged through
 *       LDS chunk by chunk),
 *   3 = tiled with a split tail (whole rounds of four-row workgroups, the remaining rows as two-row workgroups in a
 *       second launch) whenever one image fills a whole round of the resident slots, else as 0; what the rule picks
 *       for one 268x640-class frame (149 -> 142 us).
 * All of them produce BIT-IDENTICAL planes (same taps in the same order per phase).  The numbering has a gap: 1 and 2
 * were a streaming form (weights LDS-resident, autonomous waves), which measured +-0 through the frame and was removed
 * (EXPERIMENTS.md, round 6). */
int tg_convt3x3s2_z_fwd_form(const float* x, int64_t x_nstride, const float* w_packed,
                             const float* bias, const float* wz, int cz, float* z,
                             int64_t z_nstride, int n, int cin, int cout, int h, int w, int act,
                             int form, tg_stream_t stream);
/* The Z mode of a 64 -> 64 channel ConvTranspose2d in the Winograd domain: the same quantity as
 * tg_convt3x3s2_z_fwd_form (the 9*cz tap planes of the output conv over act(convT(x) + bias), in the same
 * (n, 32, 2h, 2w) buffer), with F(2,2) along x and y over 2x2 input tiles -- 25 products per tile instead of 36 --
 * on 16x16x4 fp32 MFMAs.  Not bit-identical to the direct form (different summation order; within 1e-5 of the fp64
 * composition like it).  w_wino: tg_convt_pack_wino of the direct form's packed weights (tg_conv3x3_pack(transposed=1),
 * TG_CONVT_WINO_FLOATS floats out); wz: tg_convt_pack_wz.  cin, cout <= 64 (zero-padded to 64), cz <= 3.
 * split: -1 the library's rule, 0 one launch, 1 whole rounds of resident workgroups (two per CU) + a remainder launch
 * whenever one image has a whole round; every form gives the same planes bit for bit, and so do n = 2 and two n = 1
 * calls.  The frame plan uses it for its Z-mode layer when nf = 64 (TG_CONVTZ_WINO=0 in lab builds: the direct form). */
#define TG_CONVT_WINO_FLOATS (16 * 64 * 64)
int tg_convt_pack_wino(const float* w_packed, float* w_wino, int cin, int cout, tg_stream_t stream);
int tg_convt3x3s2_z_wino_fwd(const float* x, int64_t x_nstride, const float* w_wino, const float* bias,
                             const float* wz, int cz, float* z, int64_t z_nstride, int n, int cin, int cout,
                             int h, int w, int act, int split, tg_stream_t stream);
int tg_convout_tail(const float* z, int64_t z_nstride, int cz, const float* bias,
                    const float* up_src, int up_mode, int up_scale, float* y,
                    int64_t y_nstride, uint8_t* u8_out, int n, int h, int w,
                    tg_stream_t stream);
/* The same with the kernel form chosen by the caller: -1 the library's rule (four pixels per thread wherever w % 4 == 0
 * and the planes are 16-byte aligned), 0 one HR pixel per thread, 1 four (TG_E_SHAPE if the shape does not allow it).
 * Both forms accumulate every output in the same order: bit-identical (tests/test_hip_parity.py). */
int tg_convout_tail_form(const float* z, int64_t z_nstride, int cz, const float* bias,
                         const float* up_src, int up_mode, int up_scale, float* y,
                         int64_t y_nstride, uint8_t* u8_out, int n, int h, int w, int form,
                         tg_stream_t stream);

/* ------------------------------------------------------------------------
 * 3x3 conv with a tiny output-channel count (cout <= 4), direct fp32 VALU
 * kernel (an MFMA tile would be >90 % padding).  Replaces FNet.flow[2]
 * (32->2, +tanh*24, tecogan_nets.py:65,80) and SRNet.conv_out (64->3,
 * tecogan_nets.py:131) with the `out += upsample_func(lr_curr)` residual
 * (:145) fused: up_mode/up_scale describe how `up_src` (n, cout, h/up_scale,
 * w/up_scale) is up-sampled and added.  w_oihw is the plain (cout,cin,3,3).
 * ---------------------------------------------------------------------- */
int tg_conv3x3_small_fwd(const float* x, int64_t x_nstride, const float* w_oihw,
                         const float* bias, const float* up_src, int up_mode,
                         int up_scale, float* y, int64_t y_nstride, int n,
                         int cin, int cout, int h, int w, int act,
                         tg_stream_t stream);
/* The same launch additionally writing the result as an (h, w, cout) uint8 frame --
 * float32_to_uint8 (codes/utils/data_utils.py:80-87: round-half-even, clip) of the fp32 value
 * it stores in y -- so FRNet.infer_sequence's per-frame quantise pass and its re-read of the
 * HR frame disappear.  Needs n == 1, w % 4 == 0 and 16-byte aligned planes:
 * tg_conv3x3_small_can_fuse_u8 tells; otherwise call tg_quantize_u8_hwc on y. */
int tg_conv3x3_small_fwd_u8(const float* x, int64_t x_nstride, const float* w_oihw,
                            const float* bias, const float* up_src, int up_mode,
                            int up_scale, float* y, int64_t y_nstride, uint8_t* u8_out,
                            int n, int cin, int cout, int h, int w, int act,
                            tg_stream_t stream);
int tg_conv3x3_small_can_fuse_u8(const float* x, int64_t x_nstride, const float* y,
                                 int64_t y_nstride, int n, int cin, int h, int w);
/* y = act(conv3x3(x) + bias) + res with an explicit residual tensor (n, cout, h, w) -- the training step
 * computes the bicubic frame of `out += upsample_func(lr_curr)` (tecogan_nets.py:145) once per step instead
 * of 16 taps per pixel in every epilogue.  w % 4 == 0, 16-byte aligned planes.  (Launches of a few
 * workgroups -- the training frames -- run as 4-row tiles with the waves of a workgroup splitting the input
 * channels, with or without a residual: tg_conv3x3_small_fwd picks that form by itself.) */
/* The mirror image: cin <= 4, any number of output channels, no bias / activation, optional ReLU mask
 * (y = relu_mask > 0 ? conv : 0) -- the data gradient of a cout <= 4 head (conv_out 64 -> 3, the flow head
 * 32 -> 2): w_oihw = (cout, cin, 3, 3) of THIS op, i.e. the layer's weights with the channel roles
 * swapped and the taps rotated by 180 degrees.  w % 4 == 0, 16-byte aligned planes. */
int tg_conv3x3_fewin_fwd(const float* x, int64_t x_nstride, const float* w_oihw, const float* relu_mask,
                         int64_t mask_nstride, float* y, int64_t y_nstride, int n, int cin, int cout,
                         int h, int w, tg_stream_t stream);
int tg_conv3x3_small_fwd_res(const float* x, int64_t x_nstride, const float* w_oihw, const float* bias,
                             const float* res, int64_t res_nstride, float* y, int64_t y_nstride, int n,
                             int cin, int cout, int h, int w, int act, tg_stream_t stream);

/* ------------------------------------------------------------------------
 * Fused: reflect-pad(bottom/right) -> scale * upsample -> backward_warp ->
 * space_to_depth.   Replaces tecogan_nets.py:238-250 (step) / :189,203,208
 * (forward_sequence):
 *   lr_flow (n, 2, fh, fw) with fh = h/8*8, fw = w/8*8 (FNet output);
 *   hr_prev (n, c, s*h, s*w);
 *   out[n, (sy*s+sx)*c + ch, oy, ox] = warp(hr_prev, s*up(pad(lr_flow)))[n, ch, oy*s+sy, ox*s+sx]
 * written at out + n*out_nstride (so it can land in the channel slice of the
 * SRNet input buffer).  hr_flow_out (n,2,s*h,s*w) may be NULL; when given the
 * up-sampled flow is also stored (training needs it for D and for backward).
 * ---------------------------------------------------------------------- */
int tg_flowup_warp_s2d_fwd(const float* lr_flow, int fh, int fw,
                           const float* hr_prev, float* out,
                           int64_t out_nstride, float* hr_flow_out, int n,
                           int c, int h, int w, int scale, int up_mode,
                           tg_stream_t stream);
/* Measurement aid (bench.py roofline_warp*.copy_ceiling; no counterpart in the reference): a float4 grid-stride copy of
 * `bytes` (read once, written once) launched with the given grid -- the fused warp kernel's own -- so that its HBM
 * fraction can also be read against what a plain copy of the same size reaches on this part. */
int tg_copy_ceiling(const void* src, void* dst, int64_t bytes, int blocks, int threads, tg_stream_t stream);

/* backward_warp(x, flow): codes/utils/net_utils.py:50-82 (grid_sample bilinear,
 * border, align_corners=True; flow ch0 = x, ch1 = y, in pixels). */
int tg_backward_warp_fwd(const float* x, const float* flow, float* y, int n,
                         int c, int h, int w, tg_stream_t stream);

/* space_to_depth(x, s): net_utils.py:36-47.  x (n,c,h,w) -> y (n,s*s*c,h/s,w/s) */
int tg_space_to_depth(const float* x, float* y, int64_t y_nstride, int n, int c,
                      int h, int w, int scale, tg_stream_t stream);

/* upsample_func: BicubicUpsampler.forward net_utils.py:133-156 /
 * F.interpolate bilinear :86-89.  x (nc,h,w) -> y (nc, s*h, s*w), y = mul * up(x). */
int tg_upsample_fwd(const float* x, float* y, int nc, int h, int w, int scale,
                    int up_mode, float mul, tg_stream_t stream);

/* nn.MaxPool2d(2,2) floor mode: tecogan_nets.py:28,35,42.  y (nc, h/2, w/2) */
int tg_maxpool2_fwd(const float* x, float* y, int nc, int h, int w,
                    tg_stream_t stream);

/* float32_to_uint8 + CHW->HWC: codes/utils/data_utils.py:80-87 and the
 * transpose at tecogan_nets.py:281.  x (c,h,w) fp32 -> y (h,w,c) uint8,
 * y = uint8(clip(rint(x*255), 0, 255)), rint = round-half-even. */
int tg_quantize_u8_hwc(const float* x, uint8_t* y, int c, int h, int w,
                       tg_stream_t stream);

/* uint8 HWC frames -> fp32 CHW in [0,1], the `gt.permute(0,3,1,2).float() / 255.0` of
 * BaseModel.prepare_inference_data (codes/models/base_model.py:112).
 * x (n,h,w,c) uint8 -> y (n,c,h,w) fp32. */
int tg_dequantize_u8_hwc(const uint8_t* x, float* y, int n, int c, int h, int w,
                         tg_stream_t stream);

/* Planar YUV 4:2:0, 8 bit (I420), in and out of FRNet.infer_stream; the reference has no
 * counterpart (it reads and writes PNG folders only).  A frame is the Y plane h*w, then U, then V, each ch*cw with
 * ch = ceil(h/2), cw = ceil(w/2), tightly packed; frame k of a batch starts at k * (h*w + 2*ch*cw).
 *   matrix: Kr, Kb = 0.299, 0.114 (BT601) or 0.2126, 0.0722 (BT709); Kg = 1 - Kr - Kb.
 *   full_range 0: Y offset 16, scales 219 (luma) and 224 (chroma); 1: offset 0, scales 255.
 *   siting: where a chroma sample sits in its 2x2 luma block: in the centre (y4m C420jpeg), or on the left luma
 *   column and between the rows (y4m C420mpeg2).
 * Any other enum value, a null pointer or n < 1 is TG_E_ARG. */
enum { TG_YUV_BT601 = 0, TG_YUV_BT709 = 1 };
enum { TG_YUV_CENTER = 0, TG_YUV_LEFT = 1 };
/* yuv (n frames I420, h x w, any h, w >= 2) -> rgb_chw (n,3,h,w) fp32 in [0,1]: chroma up-sampled bilinearly in exact
 * integers (weights (1,3)/(3,1) per axis around a centred sample, (4)/(2,2) along a co-sited axis, indices clamped),
 * one fp32 matrix step, clamp.  Within 2e-6 of the fp64 formula. */
int tg_yuv420_to_rgb_f32(const uint8_t* yuv, float* rgb_chw, int n, int h, int w, int matrix, int full_range,
                         int siting, tg_stream_t stream);
/* rgb_hwc (n,H,W,3) uint8 -> yuv (n frames I420, H x W; H and W even, else TG_E_ARG), exact integer arithmetic:
 * Q = rint(M * 65536); Y = clip((Q_Y.RGB + (yo << 16) + 2^15) >> 16); chroma from the sum S of the 2x2 block
 * (centre: shift 18) or of (1,2,1) x 2 rows around the left column, x-1 clamped (left: shift 19), plus 128. */
int tg_rgb_u8_to_yuv420(const uint8_t* rgb_hwc, uint8_t* yuv, int n, int H, int W, int matrix, int full_range,
                        int siting, tg_stream_t stream);

/* Planar YUV 4:2:0 at 10 or 12 bits per sample (y4m C420p10 / C420p12).  A sample is a 16-bit
 * little-endian word holding `depth` significant bits; a frame is I420's layout with 2-byte samples, 2 (h*w + 2*ch*cw)
 * bytes.  matrix, full_range and siting are the enums above.  Limited range at depth d: yo = 16 << (d-8), ys = 219 <<
 * (d-8), cs = 224 << (d-8), chroma mid value 128 << (d-8); full range: yo = 0, ys = cs = 2^d - 1, mid 2^(d-1).
 * depth other than 10 or 12, a yuv pointer that is not 2-byte aligned (or an fp32 pointer that is not 4-byte aligned), a
 * null pointer, an unknown enum value or n < 1 is TG_E_ARG, without a launch. */
/* yuv (n frames, h x w, any h, w >= 2) -> rgb_chw (n,3,h,w) fp32 in [0,1], as tg_yuv420_to_rgb_f32: the same integer
 * chroma up-sampling (weights sum to 16), one fp32 matrix step with the depth's yo, ys, cs and mid, clamp.  A sample
 * above 2^depth - 1 is read as 2^depth - 1.  Within 2e-6 of the fp64 formula. */
int tg_yuv420p16_to_rgb_f32(const uint16_t* yuv, float* rgb_chw, int n, int h, int w, int depth, int matrix,
                            int full_range, int siting, tg_stream_t stream);
/* rgb_chw (n,3,H,W) fp32 (the layout of the HR state) -> yuv (n frames, H x W; H and W even, else TG_E_ARG).  One
 * float step per value, q = (int) rintf(c * 65535.0f) with c = v > 0 ? v : 0 (NaN gives 0), then c < 1 ? c : 1; then
 * exact 64-bit integers: Q = rint(M_d * 2^24), M_d the matrix with ys/65535 and cs/65535; Y = clip((Q_Y.q + (yo << 24) +
 * 2^23) >> 24, 0, 2^d - 1); chroma from the sum S of q over the 2x2 block (centre: shift 26) or over (1,2,1) x 2 rows
 * around the left column, x-1 clamped (left: shift 27), plus the mid value, clipped alike. */
int tg_rgb_f32_to_yuv420p16(const float* rgb_chw, uint16_t* yuv, int n, int H, int W, int depth, int matrix,
                            int full_range, int siting, tg_stream_t stream);

/* Planar YUV 4:2:0, 4:2:2 and 4:4:4 at 8, 10 or 12 bits per sample, and the BT.2020 matrix.  A
 * frame is the Y plane h*w, then U, then V, each ceil(h/sy) x ceil(w/sx) with (sx, sy) = (2,2) (420), (2,1) (422),
 * (1,1) (444), tightly packed; a sample is a byte at depth 8 and a 16-bit little-endian word above it (one above
 * 2^depth - 1 is read as 2^depth - 1).  matrix, full_range and siting are the enums above, plus TG_YUV_BT2020
 * (non-constant luminance: Kr, Kb = 0.2627, 0.0593), which ONLY the three functions below accept.  The arithmetic is
 * the one of the four 4:2:0 functions above with a subsampled axis switched on or off, and at chroma 420 with BT601 /
 * BT709 the results are theirs bit for bit: those four run their own argument checks and then the same kernels (one
 * template per direction, these are the only yuv kernels).  The integer tables rint(M * 2^16) / rint(M_d * 2^24) are computed on the host in
 * fp64 from (Kr, Kb).  Samples carry whatever transfer function the material has (PQ and HLG included): code values
 * pass through, nothing is linearised.
 *   in:  chroma to sixteenths in exact integers -- a subsampled axis by its rule above ((1,3)/(3,1) vertically, the
 *        siting's rule horizontally), an axis that is not subsampled times 4 (a 4:4:4 sample is 16 c) -- every index
 *        clamped into the plane, then the one fp32 matrix step and the clamp.
 *   out: Y as above.  A chroma sample is dot(Q row, tap-weighted RGB sum) + (mid << sh) + (1 << (sh-1)), clamped and
 *        then shifted by sh = 16 + t (8 bit) or 24 + t (10 | 12 bit), 2^t the total tap weight: 444 the pixel itself
 *        (t = 0, the siting is not looked at); 422 centre the two pixels of the pair (t = 1), 422 left (1,2,1) over
 *        x-1, x, x+1 of the row with x-1 clamped to 0 (t = 2); 420 as above (t = 2 centre, 3 left).
 * A null pointer, an unknown enum value, a depth other than 8 | 10 | 12 (8 | 10 | 12 in, 10 | 12 for the 16-bit
 * output), n < 1, an fp32 pointer that is not 4-byte aligned, a pointer to 16-bit samples that is not 2-byte aligned,
 * or a shape outside the lines below is TG_E_ARG, without a launch. */
enum { TG_YUV_BT2020 = 2 };
enum { TG_YUV_420 = 0, TG_YUV_422 = 1, TG_YUV_444 = 2 };
/* yuv (n frames, h x w, any h, w >= 2; uint8_t samples at depth 8, uint16_t at 10 | 12) -> rgb_chw (n,3,h,w) fp32 in
 * [0,1] */
int tg_yuv_planar_to_rgb_f32(const void* yuv, float* rgb_chw, int n, int h, int w, int chroma, int depth, int matrix,
                             int full_range, int siting, tg_stream_t stream);
/* rgb_hwc (n,H,W,3) uint8 -> yuv (n frames of bytes, H x W).  420: H and W even; 422: W even; 444: any H, W >= 1. */
int tg_rgb_u8_to_yuv_planar(const uint8_t* rgb_hwc, uint8_t* yuv, int n, int H, int W, int chroma, int matrix,
                            int full_range, int siting, tg_stream_t stream);
/* rgb_chw (n,3,H,W) fp32 -> yuv (n frames of 16-bit samples at depth 10 | 12, H x W; the shapes of the line above),
 * through the one float step q = (int) rintf(clamp(v) * 65535.0f) of tg_rgb_f32_to_yuv420p16. */
int tg_rgb_f32_to_yuv_planar16(const float* rgb_chw, uint16_t* yuv, int n, int H, int W, int chroma, int depth,
                               int matrix, int full_range, int siting, tg_stream_t stream);
/* Host query, no device call: the tables that all seven functions above hand to their kernels (one kernel template
 * per direction; the four 4:2:0 functions launch its 420 forms).  depth 8 | 10 | 12, matrix and full_range as above
 * (TG_YUV_BT2020 included); anything else, or a null pointer, is TG_E_ARG.
 *   q: rint(M * 2^16) (depth 8) or rint(M_d * 2^24), rows Y, Cb, Cr (q[0..8]); then yo, the chroma mid value, 2^depth - 1
 *   f: the fp32 gains of the input direction's matrix step: ky = 1/ys, then rv, gu, gv, bu per sixteenth of a code */
int tg_yuv_tables(int depth, int matrix, int full_range, int q[12], float f[5]);

/* Semi-planar YUV: what hardware decoders and encoders exchange -- NV12 / NV16 / NV24 at 8 bits,
 * P010 / P012, P210 / P212, P410 / P412 above.  A frame is the Y plane h*w, then ONE chroma plane of ceil(h/sy) rows of
 * 2 * ceil(w/sx) samples, sample 2c of a row U[r, c] and sample 2c + 1 V[r, c], tightly packed: the sample count of the
 * planar frame of the same chroma.  A sample is a byte at depth 8 and above it a 16-bit little-endian word that holds
 * code << (16 - depth): read as word >> (16 - depth) (the low bits are ignored, so nothing exceeds 2^depth - 1), written
 * with the low bits zero.  Everything else -- enums, tables, siting, taps, the one fp32 step on the way in, the exact
 * integers on the way out -- is the planar functions': these three launch the same two kernel templates with the
 * chroma layout switched, the samples equal those of the planar function on the relaid frame bit for bit, and the
 * argument lists, shapes, refusals (TG_E_ARG without a launch) and alignment rules are the planar ones. */
int tg_yuv_semiplanar_to_rgb_f32(const void* yuv, float* rgb_chw, int n, int h, int w, int chroma, int depth,
                                 int matrix, int full_range, int siting, tg_stream_t stream);
int tg_rgb_u8_to_yuv_semiplanar(const uint8_t* rgb_hwc, uint8_t* yuv, int n, int H, int W, int chroma, int matrix,
                                int full_range, int siting, tg_stream_t stream);
int tg_rgb_f32_to_yuv_semiplanar16(const float* rgb_chw, uint16_t* yuv, int n, int H, int W, int chroma, int depth,
                                   int matrix, int full_range, int siting, tg_stream_t stream);

/* Motion-adaptive deinterlacing of planar YUV (the reference has no counterpart): interlaced
 * frames in, progressive frames out, same layout and sample type as tg_yuv_planar_to_rgb_f32 takes.  The
 * specification is tests/deinterlace_ref.py and the samples are equal: an edge-directed line average over three
 * directions, bounded by a three-field motion measure; exact integers, no parameters, causal (only the frame before).
 *   A frame holds two fields, p = 0 the earlier.  tff = 1: the earlier field owns the even rows.  par = p ^ (tff ? 0 : 1).
 *   Every plane alike (ph x pw).  Row r with r % 2 == par: cur[r].  A missing row r: a = cur[r-1] (cur[r+1] at the top),
 *   b = cur[r+1] (cur[r-1] at the bottom), x indices clamped into the row; for d = 0, -1, +1:
 *   score_d = sum_{e=-1..1} |a[x+d+e] - b[x-d+e]|, candidate (a[x+d] + b[x-d] + 1) >> 1, sp = the candidate of the
 *   smallest score (a later d only when strictly smaller).  Without a frame before: sp.  Else tp = (r, x) of the field
 *   one back (cur for p = 1, the frame before for p = 0), m = max(|a[x] - prev a-row[x]|, |b[x] - prev b-row[x]|),
 *   out = min(max(sp, tp - m), tp + m).  A 16-bit word above 2^depth - 1 is read as 2^depth - 1.
 * frames: k + 1 frames, the frame before and then the k frames (with has_prev == 0 the first is never read and the
 * outputs of frames[1] are spatial only); out: cnt frames.  Output j is field f = first_field + j * step counted from
 * frames[1]: frame 1 + f / 2, p = f % 2.  step 1 (field rate) | 2 (one output per frame); first_field 0 | 1; the last
 * field lies inside the k frames.  h even and >= 4 (a multiple of 4 at 420), w >= 2.  ONE launch for all planes and
 * frames; 16-byte accesses per plane where its width, its place in a frame and both bases are multiples of 16 bytes,
 * sample by sample otherwise, with equal results.  A null pointer, an unknown enum, a flag that is not 0 | 1, a
 * 16-bit pointer that is not 2-byte aligned, k or cnt < 1 or a field window outside the frames is TG_E_ARG, without a
 * launch; more than 2 GiB on either side, or cnt above 65535, is TG_E_SHAPE. */
int tg_deinterlace_planar(const void* frames, void* out, int k, int h, int w, int chroma, int depth, int tff,
                          int has_prev, int first_field, int step, int cnt, tg_stream_t stream);

/* PNG files written on the device: what the reference's save_sequence does with cv2.imwrite
 * (codes/utils/data_utils.py), without the host's zlib.  The specification is tests/png_ref.py and the bytes are
 * equal: 8-bit RGB, no interlace, one IDAT; per row the filter type (adaptive: the one of None, Sub, Up, Average,
 * Paeth with the smallest sum of |int8(byte)|, the lowest on a tie; none: type 0); the filtered stream in segments of
 * 32768 bytes, each deflated on its own with Huffman codes only (a dynamic block and an empty stored block, or one
 * stored block when that is not larger).  No LZ77 matches, so files are larger than zlib's (tg_png_encode_lz_u8 below
 * adds them).
 *   rgb_hwc (n,h,w,3) uint8.  Frame k's complete file starts at out + k * out_stride (any alignment), its length goes
 *   to sizes[k] (8-byte aligned); bytes past it inside the stride are unspecified, bytes outside
 *   [out, out + n * out_stride) are never written.  out_stride is at least tg_png_capacity(h, w), the bytes a frame
 *   needs when every segment is stored.  workspace: at least tg_png_workspace_bytes(n, h, w) bytes, any alignment.
 *   Four launches on `stream`, ordered by the stream alone.
 * Null pointers, h or w < 1, n outside 1..65535, a bad filter: TG_E_ARG; h * (3 w + 1) >= 2^31 or a stride below the
 * capacity: TG_E_SHAPE (the two size queries return -1 then).  Nothing is launched then. */
enum { TG_PNG_FILTER_NONE = 0, TG_PNG_FILTER_ADAPTIVE = 1 };
int64_t tg_png_capacity(int h, int w);
int64_t tg_png_workspace_bytes(int n, int h, int w);
int tg_png_encode_u8(const uint8_t* rgb_hwc, int n, int h, int w, int filter, uint8_t* out, int64_t out_stride,
                     int64_t* sizes, void* workspace, tg_stream_t stream);

/* The same files with LZ77 matches; the specification is tests/png_lz_ref.py and the bytes are
 * equal.  File layout, filtering, segments, checksums and tg_png_capacity are tg_png_encode_u8's; only a segment's
 * deflate differs.  The segment is its own window: per position the up to 4 nearest earlier positions with the same
 * 16-bit hash of their four bytes are compared, the longest match (at most 258 bytes, the nearest on a tie) is taken
 * if it has 4 bytes or more (exactly 4 only up to distance 4096), the parse is greedy, and the segment is written as
 * the smallest of one stored block, tg_png_encode_u8's Huffman-only block and the LZ block (a dynamic block with
 * literal/length and distance codes plus the empty stored block), the earlier one on a tie.  So no file is longer
 * than tg_png_encode_u8's, and a frame without a match is the same file.
 *   Arguments, placement rules and error codes are tg_png_encode_u8's; workspace: at least
 *   tg_png_lz_workspace_bytes(n, h, w) bytes, any alignment: 256 KiB more per segment (the sorted keys, later the
 *   tokens, and the matches), about 5 times tg_png_workspace_bytes -- 165 MB against 33 MB for 8 frames of 536x1280.
 *   Eight launches on `stream`, ordered by the stream alone. */
int64_t tg_png_lz_workspace_bytes(int n, int h, int w);
int tg_png_encode_lz_u8(const uint8_t* rgb_hwc, int n, int h, int w, int filter, uint8_t* out, int64_t out_stride,
                        int64_t* sizes, void* workspace, tg_stream_t stream);

/* Scene cuts of FRNet.infer_stream, decided on the device; the reference has no counterpart (its
 * test sets are single-shot clips).  The formula is the specification, tests/scene_cut_ref.py restates it in numpy and
 * the three outputs must be equal bit for bit.
 *   frames (n + 1, 3, h, w) fp32, 4-byte aligned: the frame before the batch, then the batch.  Per value
 *   q = clamp(floor(fma(x, 255, 0.5)), 0, 255), NaN -> 0; luma Y = (77 R + 150 G + 29 B + 128) >> 8.  For pair j (frame
 *   j + 1 of `frames` against frame j), N = h * w:
 *     sad[j]   = sum |Y - Y'| over the pixels;
 *     hdist[j] = sum over the 32 bins b of |H[b] - H'[b]|, H[b] = pixels with Y >> 3 == b (at most 2N);
 *     flags[j] = forced[j] != 0 || (detect && sad[j] >= s_min && hdist[j] >= d_min).
 *   forced: n bytes or NULL (none forced).  Integer sums through integer atomics: the result does not depend on the
 *   order.  workspace: 8-byte aligned, at least the bytes the size query returns for n (0 for n < 1); zeroed on `stream`
 *   by the call.  Null pointers, n < 1, h or w < 1, a misaligned or short workspace: TG_E_ARG; h * w > 2^28: TG_E_SHAPE.
 *   Nothing is launched then. */
int64_t tg_scene_cut_workspace_bytes(int n);
int tg_scene_cut_flags(const float* frames, int n, int h, int w, uint64_t s_min, uint64_t d_min, const uint8_t* forced,
                       int detect, int32_t* flags, uint64_t* sad, uint32_t* hdist, void* workspace,
                       int64_t workspace_bytes, tg_stream_t stream);
/* Zero-fill `bytes` bytes at dst (any alignment) if the int32 at `flag` (device memory, 4-byte aligned) is non-zero when
 * the launch runs; a zero flag leaves every byte as it is.  The host never reads the flag.  bytes == 0: no launch.
 * Null pointers, bytes < 0, a misaligned flag: TG_E_ARG. */
int tg_zero_if_flag(void* dst, int64_t bytes, const int32_t* flag, tg_stream_t stream);

/* The BI degradation: scripts/generate_lr_bi.m of the reference -- im2double, modcrop,
 * imresize(img, 1/scale, 'bicubic'), imwrite -- on 8-bit frames, in exact integers, one launch per batch.  scale is 2
 * or 4 (else TG_E_ARG).  The frame is cut to (h - h % scale, w - w % scale); LR pixel o of an axis reads the 4*scale
 * pixels from scale*o - 3*scale/2 on, out-of-range indices mirrored with the edge pixel repeated, with the weights
 * (-3, -9, 29, 111 | mirrored) / 256 for scale 2 and (-7, -45, -75, -49, 93, 399, 745, 987 | mirrored) / 4096 for
 * scale 4.  With N the exact separable sum and D the squared denominator the byte is clamp((2N + D) // 2D, 0, 255).
 *   pad 1: LR (h/scale, w/scale).  pad 0 (training crops that carry 2*scale GT pixels of border per side): the same
 *   with 2 LR pixels cut from every side, (h/scale - 4, w/scale - 4); needs more than 4*scale pixels per axis.
 * Outputs, either or both (the other NULL): y_u8_hwc (n, h', w', 3) uint8 and y_f32_chw (n, 3, h', w') = (float)byte /
 * 255.0f, the value a loader makes of an LR PNG.
 *   tg_downsample_bi_u8:  x_hwc (n, h, w, 3) uint8.
 *   tg_downsample_bi_f32: x_chw (n, 3, h, w) fp32, each value first taken to its byte as tg_quantize_u8_hwc does
 *   (exact for the k / 255 every loader delivers).
 * A workgroup makes TG_BI_TILE_H x TG_BI_TILE_W LR pixels. */
#define TG_BI_TILE_H 8
#define TG_BI_TILE_W 32
int tg_downsample_bi_u8(const uint8_t* x_hwc, uint8_t* y_u8_hwc, float* y_f32_chw, int n, int h, int w, int scale,
                        int pad, tg_stream_t stream);
int tg_downsample_bi_f32(const float* x_chw, uint8_t* y_u8_hwc, float* y_f32_chw, int n, int h, int w, int scale,
                         int pad, tg_stream_t stream);

/* Bicubic resize of 8-bit frames to any size, the general case of the BI degradation above: one
 * launch, exact integers, nothing in global memory between the two passes.  The weights differ per output pixel, so
 * they are arguments: per axis two tables in device memory, made on the host by the contribution algorithm
 * (ops.resample_tables; tests/resize_ref.py is the specification),
 *   idx int32 [n_out][taps]: the input pixels output pixel o reads, already mirrored;
 *   w   int16 [n_out][taps]: their weights over 2^TG_RESAMPLE_WEIGHT_BITS, every row summing to exactly that.
 * With N = sum_r sum_c v_w[oy][r] h_w[ox][c] x[v_idx[oy][r]][h_idx[ox][c]] the byte is clamp((N + 2^27) >> 28, 0, 255),
 * round-half-up on the exact value.  x_hwc (n, h_in, w_in, 3) and y_hwc (n, h_out, w_out, 3) uint8, any alignment; the
 * tables 4- and 2-byte aligned.  Every index read from a table is clamped to [0, n_in - 1] and a tile of `tile`
 * outputs stages at most tg_resample_tile_span(n_in, n_out, taps, tile) pixels along an axis (a host function: the
 * bound (tile - 1) ceil(n_in / n_out) + taps + 2 the contribution algorithm keeps, never more than n_in; -1 for an
 * argument < 1), so a wrong table gives wrong bytes and never an access out of range.
 * Null pointers, n < 1, taps outside 1..TG_RESAMPLE_MAX_TAPS: TG_E_ARG; a size < 1, h_out / h_in or w_out / w_in outside
 * [1/4, 4], a frame of 2^31 bytes or more: TG_E_SHAPE.  Nothing is launched then. */
#define TG_RESAMPLE_MAX_TAPS 18
#define TG_RESAMPLE_WEIGHT_BITS 14
int tg_resample_tile_span(int n_in, int n_out, int taps, int tile);
int tg_resample_u8(const uint8_t* x_hwc, uint8_t* y_hwc, int n, int h_in, int w_in, int h_out, int w_out,
                   const int32_t* v_idx, const int16_t* v_w, int v_taps, const int32_t* h_idx, const int16_t* h_w,
                   int h_taps, tg_stream_t stream);

/* MetricCalculator.compute_PSNR (codes/metrics/metric_calculator.py:228-244) on uint8 HWC
 * frames resident on the device: sse[f] = sum of squared differences of frame f, exact
 * (integers), on the Y channel of rgb_to_ycbcr (codes/utils/data_utils.py:56-77) when
 * y_only, else over the three RGB channels.  PSNR = 20 log10(255 / sqrt(sse / count)). */
int tg_psnr_sse_u8(const uint8_t* true_hwc, const uint8_t* pred_hwc, uint64_t* sse,
                   int frames, int h, int w, int y_only, tg_stream_t stream);
/* Y channel of rgb_to_ycbcr for n RGB triples (n,3) uint8 -> (n) uint8; exposed so the
 * conversion can be checked exhaustively against numpy. */
int tg_luma_u8(const uint8_t* rgb, uint8_t* y, int64_t n, tg_stream_t stream);

/* LPIPS v0.1, alex / net-lin, spatial=False (codes/metrics/LPIPS/models/networks_basic.py:25-99,
 * pretrained_networks.py:57-95): the AlexNet layers that have no kernel elsewhere, and the head.
 * tg_lpips_conv_fwd: Conv2d(cin, cout, ks, stride, pad) + bias + ReLU as an fp32-MFMA implicit GEMM,
 * y (n, cout, oh, ow).  Weights wt are (cin*ks*ks, cout): the Conv2d weight reshaped to (cout, K)
 * and transposed.  Images [0, n0) are read from x0, [n0, n) from x1 (x1 = NULL: all from x0).  Two
 * forms: ks 11 / stride 4 with lut != NULL reads uint8 HWC RGB images (cin 3) through the (256, 3)
 * fp32 table lut[v*3 + c] (the [-1,1] scaling and ScalingLayer); ks 5 / stride 1 with lut == NULL
 * reads fp32 NCHW.  Out-of-image taps are zero (padding of the normalised input). */
int tg_lpips_conv_fwd(const void* x0, const void* x1, int n0, const float* lut, const float* wt,
                      const float* bias, float* y, int n, int cin, int h, int w, int cout, int ks,
                      int stride, int pad, tg_stream_t stream);
/* nn.MaxPool2d(3, 2), floor mode: y (nc, (h-3)/2+1, (w-3)/2+1) */
int tg_maxpool3s2_fwd(const float* x, float* y, int nc, int h, int w, tg_stream_t stream);
/* workspace of tg_lpips_head for `frames` frames of an h x w map, bytes (-1: bad arguments) */
int64_t tg_lpips_head_workspace_bytes(int frames, int h, int w);
/* One LPIPS layer: feat_true / feat_pred (frames, c, h, w) -> res[f*5 + layer] = spatial mean of
 * sum_c lin[c] (a/(|a|+1e-10) - b/(|b|+1e-10))^2.  Deterministic (fixed-order partial sums, no
 * atomics).  total != NULL (layer 4 only): total[f] = res[f*5+0] + ... + res[f*5+4], in that order. */
int tg_lpips_head(const float* feat_true, const float* feat_pred, const float* lin, int frames, int c,
                  int h, int w, void* ws, float* res, int layer, float* total, tg_stream_t stream);

/* The official evaluation protocol's frame metrics (codes/official_metrics/metrics.py:60-73) on uint8 HWC
 * frames resident on the device.  Both work on the UNROUNDED luma Y = 16 + y'/255000 with the integer
 * y' = 65481 R + 128553 G + 24966 B, on a window of h x w pixels whose origin (y0, x0) is the same in the true
 * frames (frames, true_h, true_w, 3) and the predicted frames (frames, pred_h, pred_w, 3), so that neither the
 * protocol's top-left size-matching crop nor its crop_8x8 needs a copy.  The window must lie inside both.
 *
 * tg_ssim_y_u8: ssim[f] = mean SSIM of frame f as skimage.measure.compare_ssim computes it with its defaults
 * and data_range = max - min of the PREDICTED frame's Y over the window: 7x7 uniform window, sample
 * covariance (49/48), K1 0.01, K2 0.03, mean over the (h-6) x (w-6) positions whose window lies inside.
 * Window sums are exact integers, the formula is fp64, the mean comes from fixed-order fp64 partials: results
 * are bit-identical from run to run, for any batch split, and for a window vs a contiguous copy of it.  A
 * constant predicted frame (data_range 0) gives NaN, as numpy's 0/0 does.  h, w >= 7.
 * workspace: tg_ssim_workspace_bytes(frames, h, w) bytes (-1: bad arguments). */
int64_t tg_ssim_workspace_bytes(int frames, int h, int w);
int tg_ssim_y_u8(const uint8_t* true_hwc, const uint8_t* pred_hwc, int frames, int true_h, int true_w,
                 int pred_h, int pred_w, int y0, int x0, int h, int w, double* ssim, void* workspace,
                 size_t workspace_bytes, tg_stream_t stream);
/* tg_psnr_yfloat_sse_u8: partials[f * nb + i] = exact sum of (y'_true - y'_pred)^2 over pixels
 * [4096 i, 4096 (i+1)) of frame f's window in row-major order, nb = tg_psnr_yfloat_partials(h, w) (-1: bad
 * arguments).  A whole frame does not fit 64 bits; the caller adds the partials (wider integers or fp64):
 * PSNR = 20 log10(255 / sqrt(sum / 255000^2 / (h w))). */
int64_t tg_psnr_yfloat_partials(int h, int w);
int tg_psnr_yfloat_sse_u8(const uint8_t* true_hwc, const uint8_t* pred_hwc, int frames, int true_h, int true_w,
                          int pred_h, int pred_w, int y0, int x0, int h, int w, uint64_t* partials,
                          tg_stream_t stream);

/* tOF: dense Farneback optical flow with the one parameter set of the reference's two call sites (pyr_scale 0.5,
 * levels 3, winsize 15, iterations 3, poly_n 5, poly_sigma 1.2, flags 0) and the mean end-point error of two flow
 * fields.  Specified by DESIGN.md section 7f / tests/farneback_ref.py: a restatement of the published algorithm that
 * has NOT been compared with OpenCV.  There are no parameters.  fp32; results are bit-identical from run to run and
 * for any batch split (every image of a call is worked on independently, tiles start at the image origin).
 * h, w >= 16 everywhere; bad sizes, null pointers and a short workspace are TG_E_ARG.
 * Layouts: gray (n, h, w) uint8; level images (n, lh, lw); expansions R and update matrices M as five planes per
 * image, (n, 5, h, w): (r_y, r_x, r_yy, r_xx, r_xy) and (g11, g12, g22, h1, h2); flows (n, h, w, 2), channel 0 = x.
 *
 * The stages (tg_farneback_flow_u8 enqueues exactly these launches):
 *   tg_fb_level_size       returns the coarsest level L (0..3) of an h x w frame (negative: error) and the size of
 *                          `level` (rint(h / 2^level), half to even); host only
 *   tg_fb_gray_u8          gray = (4899 R + 9617 G + 1868 B + 8192) >> 14 of the top-left h x w of `frames` frames
 *                          stored frame_h x frame_w
 *   tg_fb_level_image      Gaussian blur of the full-resolution gray frame (reflect-101; sizes 3, 3, 9, 19 for levels
 *                          0..3) + bilinear resize to the level's size.  tmp: n * h * w floats
 *   tg_fb_polyexp          polynomial expansion (11 x 11, sigma 1.2, replicate borders) of n images
 *   tg_fb_update_matrices  r: pairs + 1 expansions, pair p = images p and p + 1; flow (pairs, h, w, 2) -> m_out
 *   tg_fb_blur_solve       15 x 15 box mean of m (replicate borders) and the 2 x 2 solve -> flow_out; box_out (NULL, or
 *                          (pairs, 5, h, w)) also receives the box means
 *   tg_fb_resize_flow      bilinear resize of flows, values times 2 */
int tg_fb_level_size(int h, int w, int level, int* level_h, int* level_w);
int tg_fb_gray_u8(const uint8_t* rgb_hwc, int frames, int frame_h, int frame_w, int h, int w, uint8_t* gray,
                  tg_stream_t stream);
int tg_fb_level_image(const uint8_t* gray, int n, int h, int w, int level, float* tmp, float* out,
                      tg_stream_t stream);
int tg_fb_polyexp(const float* img, int n, int h, int w, float* r_out, tg_stream_t stream);
int tg_fb_update_matrices(const float* r, const float* flow, float* m_out, int pairs, int h, int w,
                          tg_stream_t stream);
int tg_fb_blur_solve(const float* m, float* flow_out, float* box_out, int pairs, int h, int w, tg_stream_t stream);
int tg_fb_resize_flow(const float* flow_in, int h_in, int w_in, float* flow_out, int h_out, int w_out, int pairs,
                      tg_stream_t stream);
/* tg_farneback_flow_u8: flow_out (frames - 1, h, w, 2) = flows of the consecutive pairs of `frames` uint8 HWC frames,
 * computed on the top-left h x w of frames stored frame_h x frame_w (the protocol's size-matching crop needs no
 * copy).  workspace: tg_farneback_workspace_bytes(frames - 1, h, w) bytes (-1: bad arguments). */
int64_t tg_farneback_workspace_bytes(int pairs, int h, int w);
int tg_farneback_flow_u8(const uint8_t* rgb_hwc, int frames, int frame_h, int frame_w, int h, int w, float* flow_out,
                         void* workspace, size_t workspace_bytes, tg_stream_t stream);
/* tg_flow_epe_mean: mean_f64[i] = mean over the window (y0, x0, ch, cw) of sqrt(dx^2 + dy^2) of flow_a[i] - flow_b[i],
 * both (n, h, w, 2): the per-pixel value in fp32 (products, sum and square root each rounded once), the mean from
 * fixed-order fp64 partials (pixel i of the window goes to partial i % 1024; the partials are added as a tree). */
int tg_flow_epe_mean(const float* flow_a, const float* flow_b, int n, int h, int w, int y0, int x0, int ch, int cw,
                     double* mean_f64, tg_stream_t stream);

/* ========================================================================
 * Training side: backward kernels.
 * Conv data gradients reuse tg_conv3x3_fwd with weights packed by
 * tg_conv3x3_pack(..., transposed = 2) (rot180 + in/out swap).
 * ====================================================================== */

/* dW of Conv2d(cin,cout,3,1,1):  G[a][b][tap] (+)= sum_{n,y,x} p[n][a][y][x] * q[n][b][y+ky-1][x+kx-1]
 * with p = dZ (a = cout), q = X (b = cin); fp32 MFMA, deterministic split reduction.
 * `grad` is the (ca, cb_total, 3, 3) gradient tensor; columns [cb_off, cb_off+cb) are
 * written (two-source convs call it once per source).  workspace:
 * tg_wgrad3x3_workspace_floats(...) floats, caller owned. */
size_t tg_wgrad3x3_workspace_floats(int n, int ca, int cb_total, int h, int w);
int tg_wgrad3x3(const float* p, int64_t p_nstride, const float* q, int64_t q_nstride,
                float* grad, float* workspace, int n, int ca, int cb, int cb_total,
                int cb_off, int h, int w, int accumulate, tg_stream_t stream);

/* tg_wgrad3x3 / tg_bias_grad over a batch that lives in `nseg` (<= 64) separately allocated
 * segments of `n_per_seg` images each -- the per-frame tensors of a layer that is applied
 * once per unrolled frame (FRNet.forward_sequence, tecogan_nets.py:174-225).  p_list / q_list /
 * dy_list are HOST arrays of device pointers; they are read during the call only. */
int tg_wgrad3x3_multi(const float* const* p_list, const float* const* q_list, int nseg,
                      int64_t p_nstride, int64_t q_nstride, float* grad, float* workspace,
                      int n_per_seg, int ca, int cb, int cb_total, int cb_off, int h, int w,
                      int accumulate, tg_stream_t stream);
/* tg_wgrad3x3_multi that also delivers the layer's bias gradient: bias_grad (ca floats) (+)= sum of p over
 * images and pixels, taken from the p values the kernel stages anyway (vector staging: w % 4 == 0, aligned
 * planes; other forms run tg_bias_grad_multi themselves) -- no second pass over dZ.  That reduction takes no stride:
 * with more than one image per segment p_nstride must be the packed ca * h * w, TG_E_ARG otherwise. */
int tg_wgrad3x3_multi_bias(const float* const* p_list, const float* const* q_list, int nseg,
                           int64_t p_nstride, int64_t q_nstride, float* grad, float* bias_grad,
                           float* workspace, int n_per_seg, int ca, int cb, int cb_total, int cb_off,
                           int h, int w, int accumulate, tg_stream_t stream);
/* tg_wgrad3x3_multi for a space-to-depth embedded strided conv (see tg_conv3x3_fwd_phased): the
 * q channels come in 4 sub-pixel phases of `cphase` (multiple of 64) channels and only the taps
 * the phase owns are computed; the other entries of grad are written as 0. */
int tg_wgrad3x3_multi_phased(const float* const* p_list, const float* const* q_list, int nseg,
                             int64_t p_nstride, int64_t q_nstride, float* grad,
                             float* workspace, int n_per_seg, int ca, int cb, int h, int w,
                             int accumulate, int cphase, int taps_phase0, int taps_phase1,
                             tg_stream_t stream);
/* dW of nn.ConvTranspose2d(ci, co, 3, 2, 1, output_padding = 1) (tecogan_nets.py:119-126) straight from
 * the gradient of its output:
 *   grad[a][b][ky][kx] (+)= sum x[n][a][y][x] * dz[n][b][2y - 1 + ky][2x - 1 + kx]
 * x_list[i]: (n_per_seg, ci, h, w) inputs of the layer, dz_list[i]: (n_per_seg, co, 2h, 2w); grad in the
 * layer's own (ci, co, 3, 3) layout.  No space-to-depth copy of dZ, all nine taps in one balanced pass
 * (the phased form above spends 1 / 2 / 2 / 4 taps on its four channel blocks).  bias_grad (co floats, may be
 * NULL): the layer's bias gradient (+)= sum of dZ over images and pixels, taken from the dZ values the kernel
 * stages anyway (no second pass over the HR tensors: 637 MB per step at crop 256).  Workspace:
 * tg_wgrad3x3_convt_workspace_floats(total images, ci, co, h, w). */
size_t tg_wgrad3x3_convt_workspace_floats(int n, int ci, int co, int h, int w);
int tg_wgrad3x3_convt_multi(const float* const* x_list, const float* const* dz_list, int nseg, float* grad,
                            float* bias_grad, float* workspace, int n_per_seg, int ci, int co, int h, int w,
                            int accumulate, tg_stream_t stream);
int tg_bias_grad_multi(const float* const* dy_list, int nseg, float* db, int n_per_seg, int c,
                       int hw, int accumulate, tg_stream_t stream);
/* dx = dy * act'(.), expressed through the activation OUTPUT y (ReLU, LeakyReLU(0.2),
 * tanh*24).  dx may alias dy. */
int tg_act_bwd(const float* dy, const float* y, float* dx, int64_t n, int act,
               tg_stream_t stream);
/* db[c] (+)= sum_{n,h,w} dy */
int tg_bias_grad(const float* dy, float* db, int n, int c, int hw, int accumulate,
                 tg_stream_t stream);
/* MaxPool2d(2,2) backward; x is the pool INPUT (nc,h,w), dy (nc,h/2,w/2) */
int tg_maxpool2_bwd(const float* x, const float* dy, float* dx, int nc, int h, int w,
                    tg_stream_t stream);
/* transpose of tg_upsample_fwd: dx (nc,h,w) = up^T(mul * dy) */
int tg_upsample_bwd(const float* dy, float* dx, int nc, int h, int w, int scale,
                    int up_mode, float mul, tg_stream_t stream);
/* backward_warp backward (grid_sample bilinear/border/align_corners=True autograd):
 * dimg (n,c,h,w) and/or dflow (n,2,h,w); either may be NULL. */
int tg_backward_warp_bwd(const float* x, const float* flow, const float* dy, float* dimg,
                         float* dflow, int n, int c, int h, int w, tg_stream_t stream);
/* the same, but the image gradient is ADDED to what dimg_acc already holds (no zeroing, no separate
 * accumulation pass: the frame a warp reads usually has a gradient of its own loss term already). */
int tg_backward_warp_bwd_acc(const float* x, const float* flow, const float* dy, float* dimg_acc, float* dflow,
                             int n, int c, int h, int w, tg_stream_t stream);
/* The training unroll's pair backward_warp (net_utils.py:50-82) -> space_to_depth (net_utils.py:36-47;
 * tecogan_nets.py:208-212) as ONE launch each way: y (n, scale^2 c, h/scale, w/scale) =
 * space_to_depth(backward_warp(x, flow), scale), bit-identical to the two separate calls; backward takes the
 * gradient in that layout (dy_s2d), accumulate != 0 adds the image gradient to dimg instead of overwriting it. */
int tg_backward_warp_s2d_fwd(const float* x, const float* flow, float* y, int n, int c, int h, int w, int scale,
                             tg_stream_t stream);
int tg_backward_warp_s2d_bwd(const float* x, const float* flow, const float* dy_s2d, float* dimg, int accumulate,
                             float* dflow, int n, int c, int h, int w, int scale, tg_stream_t stream);
/* inverse of tg_space_to_depth: x (n, s*s*c, h, w) -> y (n, c, s*h, s*w) */
int tg_depth_to_space(const float* x, float* y, int n, int c, int h, int w, int scale,
                      tg_stream_t stream);
/* tg_depth_to_space whose result is the gradient of an activation OUTPUT act_y (same shape as y): the
 * result is multiplied by act'(.) on the way out (relu | lrelu 0.2, through the output as tg_act_bwd) -- one pass
 * instead of depth_to_space + act_bwd.  scale 2 | 4, w % 4 == 0, 16-byte aligned tensors
 * (tg_depth_to_space_act_bwd_supported). */
int tg_depth_to_space_act_bwd_supported(const float* x, const float* act_y, const float* y, int w, int scale);
int tg_depth_to_space_act_bwd(const float* x, const float* act_y, int act, float* y, int n, int c, int h,
                              int w, int scale, tg_stream_t stream);
/* CharbonnierLoss (optim/losses.py:31-50): *loss_accum += loss_scale * sum sqrt(d^2+eps),
 * dx = grad_scale * d / sqrt(d^2+eps)  (d = x - y); loss_accum or dx may be NULL. */
int tg_charbonnier(const float* x, const float* y, int64_t n, float eps, float loss_scale,
                   float* loss_accum, float grad_scale, float* dx, tg_stream_t stream);
/* VGGFeatureExtractor input normalisation (codes/models/networks/vgg_nets.py:29):
 * y = (x - mean[c]) / std[c];  mean == NULL means 0 (the op's backward: dx = dy / std[c]). */
int tg_channel_norm(const float* x, const float* mean, const float* std, float* y, int n,
                    int c, int64_t hw, tg_stream_t stream);
/* CosineSimilarityLoss (codes/models/optim/losses.py:53-62; F.cosine_similarity dim=1) of two
 * (n,c,h,w) feature maps, as used for the perceptual loss at vsrgan_model.py:226-241:
 * *loss_accum += loss_scale * sum_pixels(1 - cos);  da = grad_scale * d(sum_pixels(1 - cos))/da.
 * Either output may be NULL. */
int tg_cosine_loss(const float* a, const float* b, int n, int c, int64_t hw, float eps,
                   float loss_scale, float* loss_accum, float grad_scale, float* da,
                   tg_stream_t stream);
/* nn.L1Loss / nn.MSELoss selected by define_criterion (codes/models/optim/__init__.py:10-14):
 * *loss_accum += loss_scale * sum(v), dx = grad_scale * dv/dx, v = |x-y| or (x-y)^2. */
#define TG_LOSS_L1 1
#define TG_LOSS_MSE 2
int tg_pixel_loss(const float* x, const float* y, int64_t n, int mode, float loss_scale,
                  float* loss_accum, float grad_scale, float* dx, tg_stream_t stream);
/* VanillaGANLoss (optim/losses.py:6-14) against a constant target, plus the statistics
 * VSRGANModel.train logs (vsrgan_model.py:163-164,194-195):
 * stats3[0] += scale*sum(bce), [1] += scale*sum(x), [2] += scale*sum(log(sigmoid(x)+1e-8));
 * dx = grad_scale * (sigmoid(x) - target). */
int tg_bce_logits(const float* x, int64_t n, float target, float scale, float* stats3,
                  float grad_scale, float* dx, tg_stream_t stream);
/* LSGANLoss (optim/losses.py:17-28): MSE against the constant 1 / 0 target; same statistics layout
 * (stats3[0] += scale*sum((x-t)^2), [1], [2] as above), dx = grad_scale * 2 (x - target). */
int tg_lsgan_loss(const float* x, int64_t n, float target, float scale, float* stats3,
                  float grad_scale, float* dx, tg_stream_t stream);
/* torch.optim.Adam step (vsrgan_model.py:76-87), in place, `step` = 1-based count */
int tg_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr,
                 float beta1, float beta2, float eps, float weight_decay, int step,
                 tg_stream_t stream);
/* The same step behind a device-side guard: a no-op (weights and both moments untouched) when
 * *skip_if_nonzero != 0.  The training step points it at the FAULT SLOT of the network's flat gradient
 * buffer: tg_fault_to_slot adds 1 to that float when the pinned fault counter of the chained launches
 * (tg_srnet_body_fwd / _bwd) is non-zero, BEFORE the data-parallel all-reduce of the buffer -- so a fault
 * on any rank drops the update on every rank, instead of applying gradients built on stale tiles
 * (the reference has no counterpart: its layers are separate launches). */
int tg_adam_step_guarded(float* p, const float* g, float* m, float* v, int64_t n, float lr,
                         float beta1, float beta2, float eps, float weight_decay, int step,
                         const float* skip_if_nonzero, tg_stream_t stream);
int tg_fault_to_slot(const int32_t* fault_counter, float* slot, tg_stream_t stream);
int tg_axpy(float* y, const float* x, float a, int64_t n, tg_stream_t stream);
/* y[i] = x[i] / d (y may alias x): the mean of an all-reduced gradient bucket, with the IEEE division
 * DDP's `bucket / world_size` performs (base_model.py:130-136), exact for any world size. */
int tg_div_scalar(float* y, const float* x, float d, int64_t n, tg_stream_t stream);
/* BatchNorm2d (train mode, batch statistics, running stats updated with the unbiased
 * variance) + LeakyReLU(slope), tecogan_nets.py:322-340; and its backward. */
int tg_bn_lrelu_train_fwd(const float* x, const float* gamma, const float* beta,
                          float* running_mean, float* running_var, float momentum,
                          float eps, float slope, float* y, float* save_mean,
                          float* save_invstd, int n, int c, int hw, tg_stream_t stream);
int tg_bn_lrelu_train_bwd(const float* x, const float* y, const float* dy,
                          const float* gamma, const float* save_mean,
                          const float* save_invstd, float slope, float* dx,
                          float* dgamma, float* dbeta, int accumulate, float* scratch2c,
                          int n, int c, int hw, tg_stream_t stream);
/* Host only, no device work: the launch form the per-channel reductions of the two entries above take for this
 * shape (the launchers call the same rule).  *slices = equal slices of the batch reduced by separate workgroups
 * (1: one workgroup per channel; 2..8: partial results parked in y / dx and merged by a second launch; the
 * backward with dx == NULL always uses 1), *threads = workgroup size (256 | 1024) for the n / *slices images of
 * one slice.  Tests ask it which path a shape selects. */
int tg_bn_launch_geometry(int n, int c, int hw, int* threads, int* slices);
/* SyncBatchNorm halves (base_model.py:133): per-channel reductions exposed so the host can
 * exchange the packed vectors over RCCL in between.
 *   forward : tg_bn_local_stats -> stats2c = [mean | centred sum of squares] of THIS rank's
 *             slice; all-gather (world x 2c floats); tg_bn_merge_stats merges equally sized
 *             partitions with Chan's formula (no E[x^2]-mean^2 cancellation; world = 1
 *             reproduces tg_bn_lrelu_train_fwd's statistics exactly) and updates the
 *             running stats with the unbiased global variance;
 *   backward: tg_bn_lrelu_bwd_reduce -> sums2c = [sum dz | sum dz*xhat]; all-reduce(sum);
 *             tg_bn_lrelu_bwd_apply with inv_count = 1 / GLOBAL element count. */
int tg_bn_local_stats(const float* x, float* stats2c, int n, int c, int hw, tg_stream_t stream);
int tg_bn_merge_stats(const float* gathered, int world, float count_per_rank, float eps,
                      float momentum, float* mean, float* invstd, float* running_mean,
                      float* running_var, int c, tg_stream_t stream);
int tg_bn_lrelu_apply(const float* x, const float* mean, const float* invstd,
                      const float* gamma, const float* beta, float slope, float* y,
                      int n, int c, int hw, tg_stream_t stream);
int tg_bn_lrelu_bwd_reduce(const float* x, const float* y, const float* dy,
                           const float* mean, const float* invstd, float slope,
                           float* sums2c, int n, int c, int hw, tg_stream_t stream);
int tg_bn_lrelu_bwd_apply(const float* x, const float* y, const float* dy,
                          const float* mean, const float* invstd, const float* gamma,
                          const float* sums2c, float slope, float inv_count, float* dx,
                          int n, int c, int hw, tg_stream_t stream);
/* nn.Linear(k, 1) (tecogan_nets.py:375): y[r] = x[r,:].w + b, and backward */
int tg_linear1_fwd(const float* x, const float* w, const float* b, float* y, int rows,
                   int k, tg_stream_t stream);
int tg_linear1_bwd(const float* x, const float* w, const float* dy, float* dx, float* dw,
                   float* db, int rows, int k, int accumulate, tg_stream_t stream);

/* downsample_bd (codes/utils/data_utils.py:30-53): per-plane 2-D Gaussian (kernel2d:
 * ksize*ksize floats on the device, create_kernel :11-27) + stride-`scale` decimation.
 * pad = 0: valid conv (training);  pad = 1: reflect padding (testing).
 * y is (nc, oh, ow) with oh = pad ? (h-1)/scale+1 : (h-ksize)/scale+1. */
int tg_downsample_bd(const float* x, const float* kernel2d, float* y, int nc, int h,
                     int w, int ksize, int scale, int pad, tg_stream_t stream);

/* ------------------------------------------------------------------------
 * Data movement of the training step, one launch each (they replace chains of ATen slice / flip /
 * cat / zero-fill kernels):
 *   tg_time_gather     y[n][k] = x[n][idx[k]] over (n, t, inner) tensors, idx a HOST array of k <= 64
 *                      frame numbers (a negative entry writes a zero frame): the ping-pong augmentation cat(x, x.flip(1)[:, 1:])
 *                      (vsrgan_model.py:112-119), the halves hr[:, :te-1] / hr[:, te:].flip(1) of the
 *                      ping-pong loss (:246-247), data[:, :t] (tecogan_nets.py:437);
 *   tg_transpose01     y (b, a, inner) = x (a, b, inner): clip-major (n, t, ...) <-> frame-major (t, n, ...),
 *                      so that the recurrent unroll (tecogan_nets.py:196-214) reads / writes each
 *                      time step as a contiguous slice instead of copying it out;
 *   tg_stack_time      y (n, k, inner) with y[:, j] = src_host[j] (n, inner): torch.stack(frames, 1) of
 *                      the k <= 64 per-frame outputs (tecogan_nets.py:216), src_host a HOST array of
 *                      device pointers;
 *   tg_index_gather    out[i] (+)= src[idx[i]], 0 where idx[i] is outside [0, n_src): the weight
 *                      re-layouts that express ConvTranspose2d(k3,s2) backward and Conv2d(k4,s2) as
 *                      3x3 convolutions over space_to_depth tensors, and their inverse on the gradient;
 *   tg_pingpong_grad   the ping-pong loss gradient g (n, te-1, inner) routed onto the 2*te-1 frames:
 *                      +g | 0 | -flip(g);
 *   tg_d_assemble_fwd  SpatioTemporalDiscriminator's input (tecogan_nets.py:440-463): x (n*t/3, 9c, h, w)
 *                      = [frame triplets rrrgggbbb | warped triplets centre-cropped (crop) and
 *                      zero-padded (pad) | bicubic condition]; data / cond are (n, t_data|t_cond, c, h, w)
 *                      of which the first t frames are used, warped is (n*t, c, h, w);
 *   tg_d_assemble_bwd  its adjoint: g -> g_data (n, t_data, c, h, w; zero beyond t), g_warped (n*t, c, h, w).
 * ---------------------------------------------------------------------- */
/* tg_time_gather, tg_transpose01 and tg_stack_time move 16 bytes per thread: inner % 4 == 0 (tg_time_gather:
 * TG_E_SHAPE otherwise; the other two: TG_E_ARG) and every source and y 16-byte aligned (TG_E_ARG otherwise). */
int tg_time_gather(const float* x, float* y, const int* idx_host, int n, int t_in, int k,
                   int64_t inner, tg_stream_t stream);
int tg_transpose01(const float* x, float* y, int a, int b, int64_t inner, tg_stream_t stream);
int tg_stack_time(const float* const* src_host, int k, float* y, int n, int64_t inner,
                  tg_stream_t stream);
int tg_index_gather(const float* src, const int64_t* idx, float* out, int64_t n_out, int64_t n_src,
                    int accumulate, tg_stream_t stream);
int tg_pingpong_grad(const float* g, float* out, int n, int te, int64_t inner, tg_stream_t stream);
int tg_d_assemble_fwd(const float* data, int t_data, const float* warped, const float* cond,
                      int t_cond, float* x, int n, int t, int c, int h, int w, int pad, int crop,
                      tg_stream_t stream);
int tg_d_assemble_bwd(const float* g, float* g_data, int t_data, float* g_warped, int n, int t, int c,
                      int h, int w, int pad, int crop, tg_stream_t stream);

/* ------------------------------------------------------------------------
 * Training-batch assembly from an HBM-resident uint8 training set (the decoded LMDB of
 * scripts/create_lmdb.py:57: raw RGB HWC frames).  Replaces the per-sample CPU work of
 * UnpairedLMDBDataset.__getitem__ (codes/data/unpaired_lmdb_dataset.py:55-89: frame windows
 * incl. "moving first frame", crop_sequence :95-109, augment_sequence :112-129, /255) and the
 * H2D copy of the fp32 batch.  Geometry is the caller's (drawn with the reference's random
 * streams):
 *   geo (n, t, 4) int64: byte offset of the stored frame in `store`, frame width, window
 *                        row0, col0;   aug (n, 3) int32: flip axis (0 | 2 rows | 3 columns,
 *                        numpy axes of the tchw stack), temporal flip (0|1), np.rot90 count;
 *   out (n, t, c, size, size) fp32 = rot90(flip_t(flip_s(windows))) / 255.
 * ---------------------------------------------------------------------- */
int tg_gather_clips_u8(const uint8_t* store, const int64_t* geo, const int32_t* aug,
                       float* out, int n, int t, int c, int size, tg_stream_t stream);

/* ------------------------------------------------------------------------
 * RCCL exchange of the data-parallel training step (one process per GPU, xGMI).
 * Replaces DistributedDataParallel's gradient all-reduce (base_model.py:130-136), the
 * SyncBatchNorm statistics exchange (:133) and dist.all_reduce of the adaptive-D scalars
 * (vsrgan_model.py:166-173) for a host WITHOUT torch.distributed: rank 0 calls
 * tg_comm_get_unique_id and ships the 128 bytes to the other ranks over any channel it has
 * (the reference's launcher: env:// TCP, utils/dist_utils.py:8-24); every rank then calls
 * tg_comm_init_rank (collective, current HIP device).  Collectives only enqueue on `stream`.
 * RCCL is bound with dlopen at the first tg_comm_* call (the copy already mapped in the
 * process wins); a missing RCCL is TG_E_HIP, never a silent single-rank run.
 * The Python host mirror keeps the reference's own transport by default -- torch.distributed,
 * whose "nccl" backend IS this same RCCL -- because the process group's lifetime and
 * rendezvous belong to the host application (utils/dist_utils.py:init_dist); it switches to
 * these entry points with TECOGAN_COMM=c_abi.
 * ---------------------------------------------------------------------- */
#define TG_COMM_ID_BYTES 128 /* sizeof(ncclUniqueId) */
typedef struct tg_comm tg_comm;
int tg_comm_get_unique_id(uint8_t id[TG_COMM_ID_BYTES]);
int tg_comm_init_rank(const uint8_t id[TG_COMM_ID_BYTES], int world, int rank, tg_comm** out);
int tg_comm_destroy(tg_comm* comm);
int tg_comm_world(const tg_comm* comm);
int tg_comm_rank(const tg_comm* comm);
/* what RCCL ITSELF reports for the communicator (ncclCommCount, ncclCommUserRank) -- the reference reads the same from
 * torch.distributed (dist.get_world_size() / get_rank(), utils/dist_utils.py:27-34); a launcher / library mismatch shows
 * here before the first collective.  TG_E_HIP when the bound librccl lacks the two queries. */
int tg_comm_query(const tg_comm* comm, int* ranks_seen, int* rank_seen);
const char* tg_comm_library_origin(void); /* which librccl was bound ("" = none yet) */
/* in-place SUM over ranks (flat gradient bucket: 10.4 MB G / 3.3 MB D; BN backward sums) */
int tg_allreduce_sum_f32(tg_comm* comm, float* buf, int64_t count, tg_stream_t stream);
/* recv = [rank 0 | rank 1 | ...], count_per_rank floats each (SyncBN forward statistics) */
int tg_allgather_f32(tg_comm* comm, const float* send, float* recv, int64_t count_per_rank,
                     tg_stream_t stream);

/* ------------------------------------------------------------------------
 * Whole-frame plan: one call = FRNet.step (tecogan_nets.py:227-252).  The plan
 * holds only launch geometry and pointers into a caller-owned workspace and
 * caller-owned packed weights; it owns no device memory.
 * ---------------------------------------------------------------------- */
typedef struct tg_frnet_plan tg_frnet_plan;

typedef struct {
  int in_nc, out_nc, nf, nb, scale, up_mode; /* FRNet ctor, tecogan_nets.py:154 */
  int n, h, w;                               /* LR batch / size */
  int fnet_only;                             /* 1: plan and workspace for phase 1 (FNet) only */
} tg_frnet_cfg;

/* Weight table handed to the plan: device pointers to packed weights / biases
 * in the order documented in tecogan-pytorch_amd/models/networks/tecogan_nets.py
 * (FNet 14 convs, SRNet conv_in, 2*nb resblock convs, 1-2 conv_up, conv_out). */
typedef struct {
  const float* w;
  const float* b;
  const float* u;   /* tg_pack_conv3x3_wino form of the same weights, or NULL: the plan then runs the
                       layer in the direct form whatever its shape (see tg_conv3x3_prefers_wino) */
} tg_layer_weights;

size_t tg_frnet_workspace_floats(const tg_frnet_cfg* cfg);
int tg_frnet_plan_create(const tg_frnet_cfg* cfg, const tg_layer_weights* layers,
                         int n_layers, float* workspace, tg_frnet_plan** out);
void tg_frnet_plan_destroy(tg_frnet_plan* plan);
/* Fail-safe of the chained SRNet launch (tg_conv3x3_wino_chain inside the plan).  A workgroup that
 * gives up waiting for a producer tile counts a fault in a pinned-host counter the plan owns (64
 * bytes of hipHostMalloc memory, the only allocation a plan makes) and carries on, so the launch
 * always ends.  EVERY later tg_frnet_step* / tg_frnet_replay call on the plan looks at that counter
 * first (a host read, no synchronisation): the first call that sees it non-zero returns TG_E_HIP
 * ("frames since the fault are invalid") and switches the plan to one launch per layer (until it re-arms: see below);
 * calls after that run normally on the fallback.  tg_frnet_plan_chain_status does the same check
 * on demand (call it after a synchronisation: it then covers everything enqueued so far):
 * returns TG_OK / TG_E_HIP as above, *faults_total = faults since creation, *chain_active = 1
 * while the plan's shape still uses the chained launch.
 * tg_frnet_plan_set_chain_poll_limit: polls (~64 shader cycles each) a waiter makes before it
 * gives up; default 2^21 (~0.2 s).  A negative limit makes every waiter fault immediately
 * (fault injection for tests of the host's error path). */
int tg_frnet_plan_chain_status(tg_frnet_plan* plan, int* faults_total, int* chain_active);
int tg_frnet_plan_set_chain_poll_limit(tg_frnet_plan* plan, int poll_limit);
/* Recovery from a transient fault (round 6).  "For good" above is the round-5 behaviour and what
 * first_after_frames = 0 selects.  By default (64) the plan counts the frames it enqueues on the per-layer
 * fallback; after that many -- and once the GPU has passed the first of them (a hipEvent the plan creates on its
 * first fault and owns) with no new fault counted -- the one-launch body is armed again (its flags / exchange
 * buffers are re-zeroed in stream order).  A fault of the re-armed body is reported like the first one and
 * DOUBLES the wait (capped at 2^20 frames): a permanent co-tenant costs one invalid clip per back-off period,
 * a transient one costs 64 slower frames.  Results are bit-identical on either path.
 * tg_frnet_plan_chain_rearms: *rearms = how often the body was armed again, *current_wait_frames = the
 * back-off in force (0 before the first fault). */
int tg_frnet_plan_set_chain_rearm(tg_frnet_plan* plan, int first_after_frames);
int tg_frnet_plan_chain_rearms(const tg_frnet_plan* plan, int* rearms, int* current_wait_frames);
/* hold != 0: while it is set, frames enqueued on a fallen-back plan neither count towards the back-off nor arm the
 * one-launch body again -- they are guaranteed to run one launch per layer, which has no waiting workgroups and
 * cannot time out.  FRNet.infer_stream brackets the re-run of the batches a fault invalidated with it: a stream
 * re-arms mid-clip by design, and a body armed again INSIDE the re-run could fault a second time in frames that
 * are being repaired.  hold = 0 resumes the count where it stood.  No effect on a plan whose body is in use. */
int tg_frnet_plan_hold_chain_rearm(tg_frnet_plan* plan, int hold);
/* hr_out may alias nothing else; lr_curr/lr_prev (n,c,h,w), hr_prev/hr_out (n,c,s*h,s*w).
 * c = in_nc = out_nc = 3: the frame is the next call's hr_prev, and the output conv adds the up-sampled lr_curr
 * channel by channel, so tg_frnet_workspace_floats returns 0 and tg_frnet_plan_create TG_E_SHAPE for out_nc != in_nc.
 * u8_out (optional): (n, s*h, s*w, c) uint8 quantised frames (n > 1 needs the fused HR stage, which every
 * fp32 plan runs unless the lab switch TG_HR_FUSE=0 selects the unfused launches; the fp16 body at 2x ends in
 * the unfused one and takes n == 1 only). */
int tg_frnet_step(tg_frnet_plan* plan, const float* lr_curr, const float* lr_prev,
                  const float* hr_prev, float* hr_out, uint8_t* u8_out,
                  tg_stream_t stream);
/* The frame in two phases, for clip inference: FNet depends only on the LR frames, so
 * phase 1 of frame t+1 may run on a second stream while phase 2 of frame t is in flight.
 *   phases & 1: FNet(lr_curr, lr_prev) -> internal flow slot `flow_slot` (0|1)
 *   phases & 2: pad/upsample/warp/s2d + SRNet reading that slot -> hr_out (+ u8_out)
 * The two phases use disjoint workspace regions; the caller orders
 * phase1(slot) -> phase2(slot) -> next phase1(slot) with stream events. */
int tg_frnet_step_phase(tg_frnet_plan* plan, int phases, int flow_slot, const float* lr_curr,
                        const float* lr_prev, const float* hr_prev, float* hr_out,
                        uint8_t* u8_out, tg_stream_t stream);
/* Clip inference with a BATCHED flow estimator: FNet needs only the LR frames, so an
 * FNet-only plan (cfg.fnet_only = 1, cfg.n = frames per batch) estimates the flows of n
 * consecutive frame pairs in one pass -- as FRNet.forward_sequence does for training
 * (tecogan_nets.py:183-196) -- and the per-frame plan consumes them one by one:
 *   tg_frnet_step_phase(fnet_plan, 1, slot, lr[i0..i0+n), lr[i0-1..i0+n-1), ...)
 *   tg_frnet_step_srnet(frame_plan, tg_frnet_plan_flow(fnet_plan, slot) + j*2*fh*fw, lr[i0+j], ...)
 * with fh = h/8*8, fw = w/8*8. */
float* tg_frnet_plan_flow(tg_frnet_plan* plan, int flow_slot);
int tg_frnet_step_srnet(tg_frnet_plan* plan, const float* lr_flow, const float* lr_curr,
                        const float* hr_prev, float* hr_out, uint8_t* u8_out,
                        tg_stream_t stream);
/* number of kernel launches one tg_frnet_step enqueues (for reporting) */
int tg_frnet_plan_launches(const tg_frnet_plan* plan);

/* Measurement support: launches are grouped in `kinds` = distinct kernel symbols
 * (what `rocprofv3 --kernel-trace --stats` groups by).  tg_frnet_step_masked
 * enqueues only the launches whose kind bit is set in kind_mask (buffers keep
 * the contents of the last full step), so bench.py can bracket one kernel
 * class with HIP events; tg_frnet_plan_kind_stats returns that class's launch
 * count and ALGORITHMIC flops / bytes per frame. */
int tg_frnet_plan_kinds(void);
const char* tg_frnet_kind_name(int kind);
int tg_frnet_plan_kind_stats(const tg_frnet_plan* plan, int kind, int* launches,
                             double* flops, double* bytes);
int tg_frnet_replay(tg_frnet_plan* plan, const float* lr_curr, const float* lr_prev,
                    const float* hr_prev, float* hr_out, unsigned kind_mask, int reps,
                    tg_stream_t stream);
int tg_frnet_step_masked(tg_frnet_plan* plan, const float* lr_curr, const float* lr_prev,
                         const float* hr_prev, float* hr_out, uint8_t* u8_out,
                         unsigned kind_mask, tg_stream_t stream);

/* ------------------------------------------------------------------------
 * fp16 inference body of SRNet (tg_conv3x3_f16.hip): 64 -> 64 channel 3x3 layers on the
 * f16 matrix cores, fp32 accumulation, fp32 bias.  fp16 tensors are passed as uint16_t* (IEEE binary16 bits),
 * activations channels-last (n, h, w, 64), 16-byte aligned.  Every conversion rounds to nearest even.
 *   tg_conv3x3_f16_supported      1 if the two layer kernels take the shape (cin = cout = 64, n, h, w >= 1)
 *   tg_conv3x3_f16_packed_halves  fp16 elements of one packed weight tensor (0: cin / cout outside 1..64)
 *   tg_conv3x3_f16_act_halves     fp16 elements of one activation tensor (-1: bad shape)
 *   tg_conv3x3_f16_pack_weights   fp32 OIHW (transposed = 0) or IOHW (transposed = 1, ConvTranspose2d) -> packed
 *                                 fp16, cin and cout zero padded to 64; run once per weight tensor
 *   tg_conv3x3_f16_pack_input     channels [0, c1) of x1 and [0, c2) of x2 (fp32 NCHW) -> fp16 channels-last,
 *                                 c1 + c2 <= 64, the remaining channels zero
 *   tg_conv3x3_f16_fwd            y = round16(act(conv3x3(x) + bias) + res); res optional, y may alias res, not x
 *   tg_convt3x3s2_f16_fwd         y (fp32 NCHW, n x 64 x 2h x 2w, NOT rounded) = act(ConvTranspose2d(3, 2, 1, 1)(x) + bias)
 * act: TG_ACT_NONE | TG_ACT_RELU. */
int tg_conv3x3_f16_supported(int n, int cin, int cout, int h, int w);
size_t tg_conv3x3_f16_packed_halves(int cin, int cout);
int64_t tg_conv3x3_f16_act_halves(int n, int h, int w);
int tg_conv3x3_f16_pack_weights(const float* w, int cin, int cout, int transposed, uint16_t* out, tg_stream_t stream);
int tg_conv3x3_f16_pack_input(const float* x1, int64_t x1_nstride, int c1, const float* x2, int64_t x2_nstride,
                              int c2, uint16_t* y, int n, int h, int w, tg_stream_t stream);
int tg_conv3x3_f16_fwd(const uint16_t* x, const uint16_t* w_packed, const float* bias, const uint16_t* res,
                       uint16_t* y, int n, int cin, int cout, int h, int w, int act, tg_stream_t stream);
int tg_convt3x3s2_f16_fwd(const uint16_t* x, const uint16_t* w_packed, const float* bias, float* y,
                          int64_t y_nstride, int n, int cin, int cout, int h, int w, int act, tg_stream_t stream);

/* Precision of a frame plan's SRNet body.  TG_PREC_F32 (what tg_frnet_plan_create gives): every launch as before.
 * TG_PREC_F16: phase 2 packs SRNet's input to fp16 and runs conv_in, the residual blocks and the first
 * up-sampling layer through the kernels above, one launch per layer (no workgroup waits for another one:
 * tg_frnet_plan_chain_status reports chain_active = 0); FNet, the warp and everything behind the first
 * up-sampling layer stay the fp32 launches.
 *   plain      the PLAIN fp32 weights (`w`) and biases (`b`) of those layers, 2 + 2 * nb entries: conv_in (OIHW),
 *              the block convs (OIHW), the first up-sampling layer (IOHW); `u` is not read.  The plan packs them
 *              to fp16 once, in stream order, in front of the first fp16 frame; they must outlive the plan.
 *   workspace  tg_frnet_f16_workspace_bytes(cfg) bytes, 16-byte aligned, caller-owned like the fp32 workspace
 *              (0: the cfg has no fp16 form -- nf != 64, FNet-only, or not a valid cfg).
 * With TG_PREC_F32 `plain` and `workspace` are ignored and the fp32 launch list is restored exactly.  At scale 2
 * the fp16 body ends in the unfused output conv, so a uint8 output then needs n == 1 (TG_E_ARG otherwise, as for
 * the unfused fp32 HR stage): the plan never computes a frame in another precision than the one it was set to. */
#define TG_PREC_F32 0
#define TG_PREC_F16 1
size_t tg_frnet_f16_workspace_bytes(const tg_frnet_cfg* cfg);
int tg_frnet_plan_set_precision(tg_frnet_plan* plan, int precision, const tg_layer_weights* plain, int n_plain,
                                void* workspace);
int tg_frnet_plan_precision(const tg_frnet_plan* plan);

#ifdef __cplusplus
}
#endif
#endif /* TECOGAN_HIP_H */
