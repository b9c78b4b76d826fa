// Error channel, version, and the whole-frame FRNet.step plan.
#include <new>
#include <vector>

#include "tg_common.h"

namespace tg {
static thread_local char g_err[512] = "ok";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
}  // namespace tg

extern "C" int tg_version(void) { return TG_ABI_MAJOR * 100 + 1; }
extern "C" const char* tg_last_error_string(void) { return tg::g_err; }

#ifndef TG_BUILD_FLAGS_STR
#define TG_BUILD_FLAGS_STR "unknown (not built by csrc/build.sh)"
#endif
#ifndef TG_FILE_FLAGS_STR
#define TG_FILE_FLAGS_STR ""
#endif
namespace tg { int wres_lab_bits(); }
extern "C" const char* tg_build_info(void) {
  static char s[1024];
  if (!s[0])
    snprintf(s, sizeof(s), "lab=%d wres_lab_bits=%d flags=%s file_flags=%s", (int)TG_LAB, tg::wres_lab_bits(),
             TG_BUILD_FLAGS_STR, TG_FILE_FLAGS_STR);
  return s;
}

// ---------------------------------------------------------------------------
// FRNet.step plan (codes/models/networks/tecogan_nets.py:227-252): the launch
// list of one recurrent frame, resolved once per (shape, weights).  Owns no
// device memory: activations live in the caller's workspace.
// choose(): every launch decision of a frame beyond the per-layer conv form, each stated once.  Emit: accounts (dry
// run) or launches; its members are the stages, in launch order.  emit_frame(): what every entry and the dry run call.
// ---------------------------------------------------------------------------

// Launch classes = distinct kernel symbols (what rocprofv3 --stats groups by).
enum {
  K_CONV64_R2 = 0,  // conv3x3_mfma_kernel<2,2,1>
  K_CONV64_R4 = 1,  // conv3x3_mfma_kernel<4,1,2>
  K_CONV32 = 2,     // conv3x3_mfma_kernel<4,1,1>
  K_CONVT = 3,      // convt3x3s2_mfma_kernel<2|4,2>
  K_SMALL = 4,      // conv3x3_small_kernel<COUT>
  K_WARP = 5,       // flowup_warp_s2d_kernel<S,3>
  K_POOL = 6,
  K_UPSAMPLE = 7,
  K_QUANT = 8,
  K_FINAL = 9,      // splitk_finalize_kernel
  K_CONV64_KS = 10, // conv3x3_mfma_kernel<1,2,1,...,2>: in-workgroup K split (few tiles)
  K_CONVT_Z = 11,   // convt3x3s2_mfma_kernel<4,2,true>: last up-sampling layer + output-conv contraction
  K_TAIL = 12,      // convout_tail_kernel: 9-tap shift-add + residual + uint8
  K_CONV_ONESHOT = 13,  // conv3x3_oneshot_kernel: few tiles, cin <= 64, whole K range in flight
  K_CONV_WINO = 14,     // conv3x3_wino_kernel: Winograd F(2x2,3x3) form of the large 64-channel-group layers
  K_WINO_CHAIN = 15,    // conv3x3_wino_chain_kernel: SRNet's conv_in + residual blocks as ONE launch
  K_WINO_RES = 16,      // conv3x3_wino_resident_kernel: the same layers on persistent, LDS-resident workgroups (one 134x320-class frame)
  K_F16_PACK = 17,      // pack_input_f16_kernel: SRNet's two fp32 sources -> fp16 channels-last (fp16 body only)
  K_F16_CONV = 18,      // conv3x3_f16_kernel<false>: conv_in and the residual-block convs of the fp16 body
  K_F16_CONVT = 19,     // conv3x3_f16_kernel<true>: the first up-sampling layer of the fp16 body (fp32 out)
  K_COUNT = 20
};

// Layers by name: positions in the `layers` array of tg_frnet_plan_create (FNet's 14 first, then SRNet's)
struct LayerIndex {
  int conv_in = 14, up1 = 0, up2 = -1, out = 0, count = 0;         // (up2: 4x only)
  static int enc(int e, int j) { return 2 * e + j; }               // encoder block e (0..2), conv j (0 | 1)
  static int dec(int d, int j) { return 6 + 2 * d + j; }           // decoder block d (0..2), conv j
  static int flow(int j) { return 12 + j; }                        // flow.0 (32 channels), flow.1 (the flow)
  int body(int i) const { return conv_in + i; }                    // 0: conv_in, 1 + 2 b + j: block(b, j)
  int block(int b, int j) const { return body(1 + 2 * b + j); }    // residual block b, conv j
  explicit LayerIndex(int nb = 0, int scale = 2)
      : up1(body(1 + 2 * nb)), up2(scale == 4 ? up1 + 1 : -1), out(up1 + (scale == 4 ? 2 : 1)), count(out + 1) {}
};

struct tg_frnet_plan {
  tg_frnet_cfg cfg{};
  std::vector<tg_layer_weights> L;
  LayerIndex at;
  float *A = nullptr, *B = nullptr, *FLOW = nullptr, *S2D = nullptr, *U1 = nullptr, *U2 = nullptr, *PART = nullptr;
  // FNet's own buffers (phase 1 may overlap phase 2 of the previous frame)
  float *FA = nullptr, *FB = nullptr, *FPART = nullptr, *FLOW2 = nullptr;
  float* WZ = nullptr;              // packed output-conv weights for the fused HR stage
  float* WA = nullptr;              // Winograd-domain weights of the Z-mode layer (tg_convt_pack_wino)
  bool wz_ready = false, wa_ready = false;
  // the up-sampling readers at the low resolution (tg_upconv.hip): z of the reader that runs, the three tap packs
  float *UPZ = nullptr, *UPA = nullptr;
  bool upa_ready[3] = {false, false, false};
  int32_t* CHAINF = nullptr;        // per-tile flags of the chained SRNet launch (tg_conv3x3_wino_chain)
  bool chain_ready = false;         // flags zeroed
  unsigned epoch = 0;               // one per chained launch
  int chain_layers = 0;             // layers in the chained launch of this plan's shape (0: none)
  void* RESWS = nullptr;            // workspace of the LDS-resident SRNet body launch (exchange buffer + flags)
  bool res_ready = false;           // its flags zeroed
  // fail-safe of the chained launch: fault counter in pinned host memory (the kernel adds to it
  // with system scope), looked at by every later call on the plan
  int32_t* chain_err = nullptr;     // hipHostMalloc, 64 bytes; null when the allocation failed (chain then off)
  bool chain_disabled = false;      // a fault was reported: one launch per layer until the plan re-arms (below)
  int chain_faults = 0;             // faults reported so far
  int chain_poll_limit = tg::TG_CHAIN_POLL_LIMIT_DEFAULT;
  // Recovery from a TRANSIENT fault (a co-tenant that kept a workgroup off the GPU for a moment):
  // after `rearm_wait` clean per-layer frames the one-launch body is tried again; a fault of the re-armed body doubles
  // the wait (exponential back-off, capped), a permanent co-tenant therefore costs one faulted clip every 2^k * first
  // frames and never more.  rearm_first == 0: never re-arm (the round-5 behaviour).
  int rearm_first = 64, rearm_wait = 0, clean_frames = 0, rearms = 0;
  bool rearm_hold = false;          // tg_frnet_plan_hold_chain_rearm: frames enqueued meanwhile neither count as clean nor re-arm the body
  hipEvent_t rearm_fence = nullptr; // recorded behind the first per-layer frame after a report: the re-arm waits until the
  bool fence_set = false;           // GPU has passed it, so a late fault of a PRE-report launch is never blamed on the re-armed body
  // fp16 body (tg_frnet_plan_set_precision): packed fp16 weights and two channels-last activation buffers in a
  // caller-owned workspace; the plain fp32 weights they are packed from, once, in stream order
  bool f16 = false, f16_ready = false;
  std::vector<tg_layer_weights> HL;
  uint16_t *HWT = nullptr, *HA = nullptr, *HB = nullptr;
  int fh = 0, fw = 0, launches = 0;
  int st_launch[K_COUNT] = {};
  double st_flops[K_COUNT] = {}, st_bytes[K_COUNT] = {};
};

// Fail-safe of the chained launch: a host read of the pinned fault counter.  The first call that
// sees faults reports them (TG_E_HIP) and turns the chain off for the rest of the plan's life.
static int chain_poll(tg_frnet_plan* p) {
  if (!p->chain_err) return TG_OK;
  const int pending = __atomic_load_n(p->chain_err, __ATOMIC_RELAXED);
  if (pending == 0) return TG_OK;
  __atomic_fetch_sub(p->chain_err, pending, __ATOMIC_RELAXED);
  p->chain_faults += pending;
  // Faults that arrive after the report come from chained launches that were already enqueued when
  // the host noticed the first one (the frames of that period were declared invalid then): counted,
  // not reported again -- everything enqueued since the report uses one launch per layer.
  if (p->chain_disabled) return TG_OK;
  p->chain_disabled = true;
  p->clean_frames = 0;
  p->rearm_wait = p->rearm_wait ? (p->rearm_wait < (1 << 20) ? 2 * p->rearm_wait : p->rearm_wait) : p->rearm_first;
  p->fence_set = false;
  tg::set_error("chained SRNet launch: %d workgroup(s) timed out waiting for a producer tile; the frames "
                "enqueued on this plan since the previous successful check are INVALID.  The plan now runs "
                "one launch per layer (TG_WINO_CHAIN=0 selects that from the start)%s", pending,
                p->rearm_first > 0 ? " and tries the one-launch body again after a back-off of clean frames" : "");
  return TG_E_HIP;
}

// Called once per frame enqueued through phase 2 while the one-launch body is off: counts clean frames, and re-arms the
// body once the back-off has passed, no new fault has arrived, and the GPU is past the first per-layer frame.
static void chain_rearm_tick(tg_frnet_plan* p, tg_stream_t st) {
  if (!p->chain_disabled || !p->chain_err || p->rearm_first <= 0 || p->rearm_hold) return;
  if (!p->fence_set) {
    if (!p->rearm_fence && hipEventCreateWithFlags(&p->rearm_fence, hipEventDisableTiming) != hipSuccess) {
      (void)hipGetLastError(); p->rearm_fence = nullptr; p->rearm_first = 0; return;     // no fence -> never re-arm
    }
    if (hipEventRecord(p->rearm_fence, (hipStream_t)st) != hipSuccess) { (void)hipGetLastError(); return; }
    p->fence_set = true;
    return;
  }
  if (++p->clean_frames < p->rearm_wait) return;
  if (hipEventQuery(p->rearm_fence) != hipSuccess) { (void)hipGetLastError(); return; }   // not there yet: ask again next frame
  if (__atomic_load_n(p->chain_err, __ATOMIC_RELAXED) != 0) return;                        // (chain_poll counts it first)
  p->chain_disabled = false;
  p->res_ready = false;             // exchange buffers / flags are zeroed again in front of the next one-launch body
  p->chain_ready = false;
  p->rearms += 1;
}

// ---- the workspace: named regions, one size expression each -----------------------------------------------------------
static size_t align64(size_t v) { return (v + 63) & ~(size_t)63; }

// FNet's channels (tecogan_nets.py:67-82): three encoder blocks, three decoder blocks, flow.0, flow.1
static const int FNET_ENC[3] = {32, 64, 128}, FNET_DEC[3] = {256, 128, 64}, FNET_HEAD = 32, FNET_FLOW = 2;

// largest split-K partial buffer any layer of this shape asks for
static size_t fnet_partial_floats(const tg_frnet_cfg* c) {
  size_t best = 0;
  int hh = c->h, ww = c->w, cin = 2 * c->in_nc;
  auto consider = [&](int ci, int co) {
    int ks = tg_conv3x3_pick_ksplit(c->n, ci, co, hh, ww);
    if (ks > 1) { size_t v = (size_t)ks * c->n * co * hh * ww; if (v > best) best = v; }
  };
  for (int co : FNET_ENC) { consider(cin, co); consider(co, co); cin = co; hh /= 2; ww /= 2; }
  for (int co : FNET_DEC) { consider(cin, co); consider(co, co); cin = co; hh *= 2; ww *= 2; }
  consider(cin, FNET_HEAD);
  // SRNet layers pick split-K too when the frame itself is tiny
  hh = c->h; ww = c->w;
  consider((c->scale * c->scale + 1) * c->in_nc, c->nf); consider(c->nf, c->nf);
  return best;
}

// tap packs of the three readers of a decoder block's up-sampling (decoder2.0, decoder3.0, flow.0), back to back
static size_t fnet_upa_offset(int k) {
  size_t o = 0;
  for (int i = 0; i < k; ++i) o += tg_upconv_packed_floats(FNET_DEC[i], i < 2 ? FNET_DEC[i + 1] : FNET_HEAD);
  return o;
}

static const int CHAIN_MAX_LAYERS = 24;
// The regions in workspace order; tg_frnet_workspace_floats and tg_frnet_plan_create both walk them (carve).
enum { R_A, R_B, R_FLOW, R_S2D, R_U1, R_U2, R_PART, R_FA, R_FB, R_FPART, R_FLOW2, R_WZ_WA, R_CHAINF, R_RESWS, R_UPZ, R_UPA, R_COUNT };
static size_t region_floats(const tg_frnet_cfg* c, int region) {
  const size_t hw = (size_t)c->h * c->w, n = c->n;
  const size_t sr = c->fnet_only ? 0 : 1;                      // an FNet-only plan has no SRNet regions
  // the fused HR stage never writes the last nf-channel tensor: its region (U2 at 4x, U1 at 2x) holds the 9 * out_nc tap
  // planes of conv_out at a batch stride of 32 planes, whatever nf is
  const size_t zc = c->nf < 32 ? 32 : c->nf;
  switch (region) {
    case R_A: case R_B: return sr * align64(n * 64 * hw);      // SRNet ping, pong
    case R_FLOW: case R_FLOW2: return align64(n * 2 * hw);     // the two flow slots
    case R_S2D: return sr * align64(n * c->scale * c->scale * c->in_nc * hw);
    case R_U1: return sr * align64(n * (c->scale == 4 ? c->nf : zc) * 4 * hw);
    case R_U2: return c->scale == 4 ? sr * align64(n * zc * 16 * hw) : 0;
    case R_PART: return sr * align64(fnet_partial_floats(c));  // split-K partial sums, SRNet
    case R_FA: case R_FB: return align64(n * 64 * hw);         // FNet ping, pong
    case R_FPART: return align64(fnet_partial_floats(c));      // split-K partial sums, FNet
    // WZ (A operand of the fused output-conv contraction), then WA (Winograd-domain weights of the last up-sampling layer)
    case R_WZ_WA: return sr * (2048 + TG_CONVT_WINO_FLOATS);
    // int32 flags: 24 layers x 16-tile workgroups + error counter
    case R_CHAINF: return sr * align64((size_t)CHAIN_MAX_LAYERS * n * ((c->h + 1) / 2) * ((c->w + 31) / 32) + 16);
    // tg_conv3x3_wino_res.hip: exchange buffer + flags; n == 1 only
    case R_RESWS: return align64((size_t)(((sr && n == 1) ? tg::conv3x3_wino_resident_ws_bytes(c->h, c->w) : 0) + 3) / 4);
    // z of an up-sampling reader (tg_upconv.hip): 9 cout planes of its source map; flow.0's is the largest of the three,
    // 288 planes of the half map -- more than the 64-plane ping-pong regions hold
    case R_UPZ: return align64(n * 9 * FNET_HEAD * 16 * (size_t)(c->h / 8) * (c->w / 8));
    case R_UPA: return align64(fnet_upa_offset(3));
  }
  return 0;
}
// offsets of all regions; returns the floats of the whole workspace
static size_t carve(const tg_frnet_cfg* c, size_t off[R_COUNT]) {
  size_t o = 0;
  for (int r = 0; r < R_COUNT; ++r) { off[r] = o; o += region_floats(c, r); }
  return o;
}

// ---- the choices -------------------------------------------------------------------------------------------------------
// SRNet's 1 + 2*nb full-resolution layers as one chained launch (tg_conv3x3_wino_chain) when a layer
// has more 16-tile workgroups than fit on the GPU at once (768) but only a few rounds of them:
// measured against one launch per layer (tools/wino_chain_probe.py) -15 % at 2 clips of 134x320,
// -6.5 % at 4, -4.6 % at 268x640, +-0 at 8 clips, and +3..15 % (slower) for a single 134x320 clip, whose
// 670 workgroups are all resident at once and therefore cannot pipeline.  TG_WINO_CHAIN=0 / 1: never / whenever eligible.
static bool chain_wanted(long long ntile) {
  static const int v = [] { const char* e = getenv("TG_WINO_CHAIN"); return e && *e ? atoi(e) : -1; }();
  return v >= 0 ? v != 0 : ntile > 768 && ntile <= 3000;
}
// The LDS-resident form (tg_conv3x3_wino_res.hip) whenever the frame fits one 8x24 block per CU and is large
// enough for the Winograd form to be the per-layer choice (a single 134x320-class frame).  TG_WINO_RES=0
// selects the per-layer / chained launches, 1 the resident launch wherever it is supported (A/B runs, tests).
static bool resident_wanted(bool layer_prefers_wino) {
  static const int v = [] { const char* e = getenv("TG_WINO_RES"); return e && *e ? atoi(e) : -1; }();
  return v >= 0 ? v != 0 : layer_prefers_wino;     // 1: whenever supported (tests run small frames through it)
}

enum Body { BODY_LAYERS, BODY_CHAIN, BODY_RESIDENT, BODY_F16 };
// What a frame of this plan launches, beyond the per-layer conv form (Emit::conv).  A function of the plan's CURRENT
// state: the fail-safe turns the one-launch bodies off and on at run time, so every step asks again.
struct Choices {
  Body body;            // SRNet's conv_in + blocks: a launch per layer, the chained or the resident launch, or the fp16 body
  bool conv_in_front;   // conv_in runs the direct form as a launch of its own in front of a one-launch body
  int nchain;           // layers of a one-launch body
  bool ct_fold;         // the first transposed conv rides on the body's launch: no K_CONVT for it
  bool hr_fused;        // Z launch + tail instead of transposed conv(s) + output conv
  bool z_wino, z_two;   // the Z layer in the Winograd domain (same kind, same algorithmic flops); as two launches
};
static Choices choose(const tg_frnet_plan* p, bool one_launch_off) {
  const tg_frnet_cfg& c = p->cfg;
  const LayerIndex& at = p->at;
  const int n = c.n, h = c.h, w = c.w, s = c.scale, nf = c.nf, nbody = 1 + 2 * c.nb, cin0 = (s * s + 1) * c.in_nc;
  Choices ch{};
  // conv_in joins a one-launch body when it has a Winograd form itself (cin = 3 + 48 at 4x; 3 + 12 at 2x is
  // below the kernel's 16-channel stage and runs the direct form as its own launch)
  ch.conv_in_front = !(p->L[at.conv_in].u && tg_conv3x3_prefers_wino(n, cin0, nf, h, w));
  ch.nchain = nbody - (ch.conv_in_front ? 1 : 0);
  if (p->f16) {
    ch.body = BODY_F16;                    // one launch per layer, the first up-sampling layer included
  } else if (!one_launch_off && ch.nchain >= 2 && ch.nchain <= CHAIN_MAX_LAYERS) {
    const bool wino = tg_conv3x3_prefers_wino(n, nf, nf, h, w) != 0;
    bool chain = nf <= 64 && wino && chain_wanted((long long)n * tg::cdiv(h, 2) * tg::cdiv(w, 32));
    bool resident = n == 1 && resident_wanted(wino) && (ch.conv_in_front || cin0 <= 64) &&
                    tg::conv3x3_wino_resident_ok(n, nf, h, w);
    for (int i = ch.conv_in_front ? 1 : 0; i < nbody && (chain || resident); ++i) {   // every layer's pack supplied
      const tg_layer_weights& lw = p->L[at.body(i)];
      chain = chain && lw.u; resident = resident && lw.u && lw.b;
    }
    ch.body = resident ? BODY_RESIDENT : chain ? BODY_CHAIN : BODY_LAYERS;
  }
  // SRNet's first up-sampling layer rides on the resident launch (tg_conv3x3_wino_res.hip: transposed-conv tail) when
  // the plan holds its weights in that form (4x only: at 2x the single transposed conv is the Z-mode launch; the caller
  // opts in by supplying the tail's pack); the fp16 body always ends in it
  ch.ct_fold = ch.body == BODY_F16 || (ch.body == BODY_RESIDENT && s == 4 && p->L[at.up1].u && p->L[at.up1].b);
  // The HR stage as two launches instead of three and without the 64-channel HR tensor: the last ConvTranspose2d emits
  // the 27 tap planes of conv_out (tecogan_nets.py:119-131), a streaming kernel shift-adds them.  TG_HR_FUSE=0 selects
  // the unfused launches (lab / A-B).  At 2x the fused stage IS the first up-sampling layer: the fp16 body then ends in
  // the unfused output conv.  (cfg_ok: out_nc == 3, nf <= 64)
  static const int hr_fuse = TG_LAB_ENV("TG_HR_FUSE", 1);
  ch.hr_fused = hr_fuse != 0 && !(p->f16 && s == 2);
  // The Z-mode layer in the Winograd domain (tg_convt3x3s2_wino.hip: 25 products per 2x2 input tile instead of 36) where
  // it applies (cin = cout = 64); TG_CONVTZ_WINO=0 selects the direct Z form (lab / A-B).
  static const int convtz_wino = TG_LAB_ENV("TG_CONVTZ_WINO", 1);
  ch.z_wino = ch.hr_fused && convtz_wino != 0 && nf == 64;
  const int zh = s * h / 2, zw = s * w / 2;                    // input size of the last up-sampling layer
  ch.z_two = ch.hr_fused && (ch.z_wino ? tg::convt_z_wino_split_rule(n, zh, zw, -1) : tg::convt_z_split_rule(n, zh, zw, -1));
  return ch;
}
static bool one_launch_off(const tg_frnet_plan* p) { return !p->chain_err || p->chain_disabled; }
// the fused tail writes (n, H, W, c) uint8 frames for any n; the unfused quantise pass only n == 1
static bool plan_u8_ok(const tg_frnet_plan* p) { return p->cfg.n == 1 || choose(p, one_launch_off(p)).hr_fused; }

// ---- the emitter and the stages ----------------------------------------------------------------------------------------
// phase bits: 1 = FNet (lr_curr, lr_prev -> flow slot), 2 = warp + SRNet (flow slot, hr_prev -> hr_out)
struct Emit {
  tg_frnet_plan* const p;
  const tg_stream_t st;
  const unsigned mask;             // launch kinds that run
  const bool dry;
  const int phases;                // phases that run
  bool active = false;             // whether the phase the launches being issued belong to was asked for
  float* part_buf = nullptr;       // split-K partial sums of that phase
  int rc = TG_OK;
  const tg_frnet_cfg& c = p->cfg;  // shorthand of the plan's shape, from here on
  const LayerIndex& at = p->at;
  const int n = c.n, h = c.h, w = c.w, s = c.scale, nf = c.nf, s2dc = s * s * c.in_nc;
  const int64_t hw = (int64_t)h * w;
  const double px = (double)n * h * w, hpx = (double)n * s * s * hw;     // LR and HR pixels of the batch
  void begin_phase(int bit) { active = (phases & bit) != 0; part_buf = bit == 1 ? p->FPART : p->PART; }
  // account + (unless dry / masked out) launch
  template <class F> void go(int kind, double flops, double bytes, F&& fn) {
    if (rc != TG_OK) return;
    if (dry) { p->st_launch[kind] += 1; p->st_flops[kind] += flops; p->st_bytes[kind] += bytes; return; }
    if (active && (mask & (1u << kind))) rc = fn();
  }

  // conv3x3 (+bias+act) [+ MaxPool2d(2,2) when pool] of layer `layer`; y receives the final tensor.  up2: x is the
  // (cin, hh/2, ww/2) source of a bilinear x2 up-sampling the Winograd form folds into its staging (the caller has checked
  // that this layer runs that form, fnet_stage below).  Returns true when the pooled tensor was written to pool_tmp
  // instead of y: the pool folded into the Winograd kernel's epilogue has no intermediate tensor, and y may be the
  // layer's own input (the encoder blocks pool in place), which other workgroups are still reading.
  bool conv(int layer, const float* x, int64_t xns, int c1, const float* x2, int64_t x2ns, int cin, int cout, int hh,
            int ww, int act, const float* res, int64_t rns, float* y, int64_t yns, bool pool = false,
            float* pool_tmp = nullptr, bool up2 = false) {
    const tg_layer_weights lw = p->L[layer];
    const int ocb = tg_conv3x3_pick_ocb(cout);
    int kind = ocb == 32 ? K_CONV32 : tg::conv3x3_rows_per_wg(ocb, (long long)n * hh * ww) == 4 ? K_CONV64_R4 : K_CONV64_R2;
    const double mpx = (double)n * hh * ww, fl = 2.0 * cin * 9 * cout * mpx;
    double by = 4.0 * mpx * (cin + cout + (res ? cout : 0)) + 4.0 * 9 * cin * cout;
    float* const yc = pool ? pool_tmp : y;      // where the conv itself writes
    bool fpool = false;
    if (lw.u && tg_conv3x3_prefers_wino(n, cin, cout, hh, ww)) {
      // the pool is the kernel's epilogue where the map has whole 2x2 tiles: no full-resolution tensor, no K_POOL launch
      fpool = pool && !res && tg::conv3x3_wino_fuse_ok(cin, hh, ww, TG_WINO_POOL);
      const int fuse = (fpool ? TG_WINO_POOL : 0) | (up2 ? TG_WINO_UP2 : 0);
      if (fpool) by -= 4.0 * mpx * cout * 0.75;      // writes the pooled tensor
      if (up2) by -= 4.0 * mpx * cin * 0.75;         // reads the low-resolution source
      go(K_CONV_WINO, fl, by, [&] {
        return tg::conv3x3_wino_launch(x, xns, c1, x2, x2ns, lw.u, lw.b, res, rns, nullptr, 0, yc,
                                       pool && !fpool ? (int64_t)cout * hh * ww : yns, n, cin, cout, hh, ww, act, st, fuse);
      });
    } else if (up2) {      // only the Winograd form reads through the up-sampling
      if (rc == TG_OK) rc = TG_E_ARG;
      return false;
    } else {
      const int ks = res ? 1 : tg_conv3x3_pick_ksplit(n, cin, cout, hh, ww);
      if (ks == 1 && kind == K_CONV64_R2 && tg::conv3x3_uses_wg_ksplit(n, cin, cout, hh, ww))
        kind = tg::conv3x3_uses_oneshot(n, cin, cout, hh, ww) ? K_CONV_ONESHOT : K_CONV64_KS;   // launcher's rule
      if (ks > 1) {      // (the finalize launch pools)
        go(kind, fl, by, [&] {
          return tg::conv3x3_splitk_conv(x, xns, c1, x2, x2ns, lw.w, ocb, n, cin, cout, hh, ww, ks, part_buf, st);
        });
        go(K_FINAL, 0, 4.0 * mpx * cout * (ks + 1), [&] {
          return tg::conv3x3_splitk_finalize(part_buf, ks, lw.b, act, pool ? 1 : 0, y, n, cout, hh, ww, st);
        });
        return false;
      }
      go(kind, fl, by, [&] {
        return tg_conv3x3_fwd(x, xns, c1, x2, x2ns, lw.w, ocb, lw.b, res, rns, yc, pool ? (int64_t)cout * hh * ww : yns,
                              n, cin, cout, hh, ww, act, st);
      });
    }
    if (pool && !fpool)
      go(K_POOL, 0, 4.0 * n * cout * (hh * ww + (hh / 2) * (ww / 2)),
         [&] { return tg_maxpool2_fwd(yc, y, n * cout, hh, ww, st); });
    return fpool;
  }

  // The kind of the ONE launch that conv() makes of a plain layer (no pool, no residual) on the (hh, ww) map, or -1
  // where it makes two (split-K + finalize).
  int conv_single_kind(int layer, int cin, int cout, int hh, int ww) const {
    if (p->L[layer].u && tg_conv3x3_prefers_wino(n, cin, cout, hh, ww)) return K_CONV_WINO;
    if (tg_conv3x3_pick_ksplit(n, cin, cout, hh, ww) > 1) return -1;
    const int ocb = tg_conv3x3_pick_ocb(cout);
    const int kind = ocb == 32 ? K_CONV32 : tg::conv3x3_rows_per_wg(ocb, (long long)n * hh * ww) == 4 ? K_CONV64_R4 : K_CONV64_R2;
    if (kind == K_CONV64_R2 && tg::conv3x3_uses_wg_ksplit(n, cin, cout, hh, ww))
      return tg::conv3x3_uses_oneshot(n, cin, cout, hh, ww) ? K_CONV_ONESHOT : K_CONV64_KS;
    return kind;
  }
  // Whether reader k (0: decoder2.0, 1: decoder3.0, 2: flow.0) of the (sh, sw) source map runs at the low resolution
  // (tg_upconv.hip): where tg_upconv_prefers says so and the conv it replaces is one launch, so that the launch counts
  // per kind stay what they are.
  bool upconv_wanted(int layer, int cin, int cout, int sh, int sw) const {
    return tg_upconv_prefers(n, cin, cout, sh, sw) && conv_single_kind(layer, cin, cout, 2 * sh, 2 * sw) >= 0;
  }
  // conv3x3(bilinear_x2(x)) + bias + act of reader k from its (cin, sh, sw) source: tap GEMM into UPZ, then the combine.
  // No kind of their own: the GEMM is accounted as the conv launch it replaces, with that layer's algorithmic 3x3 flops
  // (as the Winograd Z layer is), the combine as the up-sampling launch it replaces.
  void upconv(int layer, int k, const float* x, int cin, int cout, int sh, int sw, int act, float* y) {
    const tg_layer_weights lw = p->L[layer];
    const double spx = (double)n * sh * sw;
    const int64_t zns = (int64_t)9 * cout * sh * sw;
    float* const a = p->UPA + fnet_upa_offset(k);
    if (rc == TG_OK && !dry && active && !p->upa_ready[k])      // once per plan, ahead of its first reader (as WZ / WA)
      p->upa_ready[k] = (rc = tg_upconv_pack(lw.w, a, cin, cout, tg_conv3x3_pick_ocb(cout), st)) == TG_OK;
    go(conv_single_kind(layer, cin, cout, 2 * sh, 2 * sw), 2.0 * cin * 9 * cout * 4 * spx,
       4.0 * spx * (cin + 9 * cout) + 4.0 * 9 * cin * cout,
       [&] { return tg_upconv_tap_gemm(x, (int64_t)cin * sh * sw, a, p->UPZ, zns, n, cin, cout, sh, sw, st); });
    go(K_UPSAMPLE, 0, 4.0 * spx * cout * (9 + 4), [&] {
      return tg_upconv_combine(p->UPZ, zns, lw.b, y, (int64_t)cout * 4 * sh * sw, n, cout, sh, sw, act, st);
    });
  }

  // ---- FNet (tecogan_nets.py:67-82), phase 1: (lr_curr, lr_prev) -> flow_buf, which it returns -------------------------
  float* fnet_stage(const float* lr_curr, const float* lr_prev, float* flow_buf) {
    begin_phase(1);
    float *A = p->FA, *B = p->FB;
    int hh = h, ww = w, cin = 2 * c.in_nc;
    const float* src = nullptr;
    for (int e = 0; e < 3; ++e) {
      const int co = FNET_ENC[e], c1 = e == 0 ? c.in_nc : cin;     // encoder1.0 reads lr_curr and lr_prev side by side
      const int64_t xns = (int64_t)c1 * hh * ww;
      conv(at.enc(e, 0), e == 0 ? lr_curr : src, xns, c1, e == 0 ? lr_prev : nullptr, e == 0 ? xns : 0, cin, co, hh, ww,
           TG_ACT_LRELU02, nullptr, 0, A, (int64_t)co * hh * ww);
      // second conv of the block + MaxPool2d: pooled result lands in A (B is scratch), or straight in B (pool folded)
      const bool in_b = conv(at.enc(e, 1), A, (int64_t)co * hh * ww, co, nullptr, 0, co, co, hh, ww, TG_ACT_LRELU02,
                             nullptr, 0, A, (int64_t)co * (hh / 2) * (ww / 2), true, B);
      hh /= 2; ww /= 2; cin = co;
      if (!in_b) { float* t = A; A = B; B = t; }   // pooled result now in B
      src = B;
    }
    // A decoder block's x2 up-sampling can be folded into the staging of the conv that reads it (decoder2.0, decoder3.0,
    // flow.0) when that conv runs the Winograd form: the block then leaves its low-resolution result in `src` and
    // there is no K_UPSAMPLE launch.  tg::conv3x3_wino_folds_up2 says where (measured: nowhere unless the form is forced).
    // Or the reader runs its matrix work on the low-resolution map itself (upconv above: a tap GEMM and a combine in the
    // place of the up-sampling launch and the conv), where upconv_wanted says so.
    bool up2 = false;      // src is the low-resolution source of the (hh, ww) map, folded into the Winograd staging
    bool low = false;      // src is that source and the reader runs at the low resolution
    // reader k of a decoder block: decoder2.0, decoder3.0, flow.0; (src, cin) -> A at (hh, ww)
    auto read_block = [&](int layer, int k, int co) {
      if (low) upconv(layer, k, src, cin, co, hh / 2, ww / 2, TG_ACT_LRELU02, A);
      else conv(layer, src, (int64_t)cin * (up2 ? (hh / 2) * (ww / 2) : hh * ww), cin, nullptr, 0, cin, co, hh, ww,
                TG_ACT_LRELU02, nullptr, 0, A, (int64_t)co * hh * ww, false, nullptr, up2);
    };
    for (int d = 0; d < 3; ++d) {
      const int co = FNET_DEC[d];
      read_block(at.dec(d, 0), d - 1, co);      // (decoder1.0 reads the encoder: neither flag is set)
      conv(at.dec(d, 1), A, (int64_t)co * hh * ww, co, nullptr, 0, co, co, hh, ww, TG_ACT_LRELU02, nullptr, 0, B,
           (int64_t)co * hh * ww);
      const int reader = d < 2 ? at.dec(d + 1, 0) : at.flow(0), rco = d < 2 ? FNET_DEC[d + 1] : FNET_HEAD;
      up2 = p->L[reader].u && tg::conv3x3_wino_folds_up2(n, co, rco, 2 * hh, 2 * ww);
      low = !up2 && upconv_wanted(reader, co, rco, hh, ww);
      if (!up2 && !low) {
        go(K_UPSAMPLE, 0, 4.0 * n * co * hh * ww * 5.0,
           [&] { return tg_upsample_fwd(B, A, n * co, hh, ww, 2, TG_UP_BILINEAR, 1.0f, st); });
        float* t = A; A = B; B = t;
      }
      hh *= 2; ww *= 2; cin = co;
      src = B;
    }
    read_block(at.flow(0), 2, FNET_HEAD);
    const tg_layer_weights lw = p->L[at.flow(1)];
    go(K_SMALL, 2.0 * FNET_HEAD * 9 * FNET_FLOW * n * hh * ww, 4.0 * n * hh * ww * (FNET_HEAD + FNET_FLOW), [&] {
      return tg_conv3x3_small_fwd(A, (int64_t)FNET_HEAD * hh * ww, lw.w, lw.b, nullptr, TG_UP_NONE, 1, flow_buf,
                                  (int64_t)FNET_FLOW * hh * ww, n, FNET_HEAD, FNET_FLOW, hh, ww, TG_ACT_TANH24, st);
    });
    return flow_buf;
  }

  // ---- where phase 2 begins: the packs derived from the plan's weights once per plan (plans are rebuilt when weights
  // change), enqueued ahead of their first reader: the fp16 body's weights, WZ from conv_out's, WA from the Z layer's
  void prepare_packs(const Choices& ch) {
    if (rc != TG_OK || dry || !(phases & 2)) return;
    if (ch.body == BODY_F16 && !p->f16_ready) {
      const int nbody = 1 + 2 * c.nb;
      const size_t wstep = tg_conv3x3_f16_packed_halves(64, 64);      // (as body_f16 reads them)
      for (int k = 0; k <= nbody && rc == TG_OK; ++k)
        rc = tg_conv3x3_f16_pack_weights(p->HL[k].w, k == 0 ? c.in_nc + s2dc : nf, nf, k == nbody ? 1 : 0,
                                         p->HWT + k * wstep, st);
      p->f16_ready = rc == TG_OK;
    }
    if (ch.hr_fused && !p->wz_ready && rc == TG_OK)
      p->wz_ready = (rc = tg_convt_pack_wz(p->L[at.out].w, p->WZ, c.out_nc, nf, st)) == TG_OK;
    if (ch.z_wino && !p->wa_ready && rc == TG_OK)
      p->wa_ready = (rc = tg_convt_pack_wino(p->L[s == 4 ? at.up2 : at.up1].w, p->WA, nf, nf, st)) == TG_OK;
  }

  // ---- pad + upsample + warp + space_to_depth (tecogan_nets.py:238-250): (flow, hr_prev) -> S2D ------------------------
  void warp_stage(const float* flow, const float* hr_prev) {
    go(K_WARP, 0, 4.0 * n * ((double)c.in_nc * s * s * hw * 2 + 2.0 * p->fh * p->fw), [&] {
      return tg_flowup_warp_s2d_fwd(flow, p->fh, p->fw, hr_prev, p->S2D, s2dc * hw, nullptr, n, c.in_nc, h, w, s, c.up_mode, st);
    });
  }

  // ---- SRNet's body (tecogan_nets.py:136-147): conv_in and the residual blocks; the result is in A ---------------------
  // layer i of the body (0 = conv_in: (lr_curr, S2D) -> A; odd = a block's conv1: A -> B; even = its conv2: B + A -> A)
  tg_wino_layer body_layer(int i, const float* lr_curr) const {
    const tg_layer_weights lw = p->L[at.body(i)];
    const bool first = i == 0, conv2 = !first && (i % 2 == 0);
    tg_wino_layer d;
    d.x = first ? lr_curr : (conv2 ? p->B : p->A);
    d.x2 = first ? p->S2D : nullptr;
    d.u_packed = lw.u; d.bias = lw.b;
    d.res = conv2 ? p->A : nullptr;
    d.y = (first || conv2) ? p->A : p->B;
    d.x_nstride = first ? c.in_nc * hw : nf * hw; d.x2_nstride = first ? s2dc * hw : 0;
    d.res_nstride = nf * hw; d.y_nstride = nf * hw;
    d.c1 = first ? c.in_nc : nf; d.cin = first ? c.in_nc + s2dc : nf;
    d.act = conv2 ? TG_ACT_NONE : TG_ACT_RELU;
    return d;
  }
  // layers [i0, i1) of the body, one launch each
  void body_layers(const float* lr_curr, int i0, int i1) {
    for (int i = i0; i < i1; ++i) {
      const tg_wino_layer d = body_layer(i, lr_curr);
      conv(at.body(i), d.x, d.x_nstride, d.c1, d.x2, d.x2_nstride, d.cin, nf, h, w, d.act, d.res,
           d.res ? d.res_nstride : 0, d.y, d.y_nstride);
    }
  }
  // the body as ONE launch, chained or resident (conv_in in front where it runs the direct form); ct_fold: up1's result in U1
  void body_one_launch(const Choices& ch, const float* lr_curr) {
    const int nchain = ch.nchain, skip = ch.conv_in_front ? 1 : 0;
    body_layers(lr_curr, 0, skip);
    tg_wino_layer cl[CHAIN_MAX_LAYERS];
    double fl = 0, by = 0;
    for (int k = 0; k < nchain; ++k) {
      const tg_wino_layer& d = cl[k] = body_layer(k + skip, lr_curr);
      fl += 2.0 * d.cin * 9 * nf * px;
      by += 4.0 * px * (d.cin + nf + (d.res ? nf : 0)) + 4.0 * 9 * d.cin * nf;
    }
    p->chain_layers = nchain;
    if (ch.body == BODY_CHAIN) {
      go(K_WINO_CHAIN, fl, by, [&] {
        if (!p->chain_ready) {
          const size_t ints = (size_t)tg_conv3x3_wino_chain_flag_ints(nchain, n, h, w);
          if (hipMemsetAsync(p->CHAINF, 0, ints * sizeof(int32_t), (hipStream_t)st) != hipSuccess)
            return tg::check_launch("wino_chain flags memset");
          p->chain_ready = true;
        }
        if (++p->epoch == 0) p->epoch = 1;
        return tg::conv3x3_wino_chain_launch(cl, nchain, n, nf, h, w, p->CHAINF, p->chain_err, p->epoch,
                                             p->chain_poll_limit, st);
      });
      return;
    }
    if (ch.ct_fold) { fl += 2.0 * nf * 9 * nf * px; by += 4.0 * px * nf * 4.0 + 4.0 * 9 * nf * nf; }
    go(K_WINO_RES, fl, by, [&] {
      if (!p->res_ready) {
        if (hipMemsetAsync(p->RESWS, 0, (size_t)tg::conv3x3_wino_resident_ws_bytes(h, w), (hipStream_t)st) != hipSuccess)
          return tg::check_launch("wino_resident workspace memset");
        p->res_ready = true;
      }
      if (++p->epoch == 0) p->epoch = 1;
      tg_wres_convt ct{p->L[at.up1].u, p->L[at.up1].b, p->U1, TG_ACT_RELU};
      return tg::conv3x3_wino_resident_launch(cl, nchain, nf, h, w, p->RESWS, p->chain_err, p->epoch << 5,
                                              p->chain_poll_limit, st, ch.ct_fold ? &ct : nullptr);
    });
  }
  // the fp16 body: one launch per layer, the first up-sampling layer included (its fp32 result lands in U1)
  void body_f16(const float* lr_curr) {
    const int nbody = 1 + 2 * c.nb;
    const size_t wstep = tg_conv3x3_f16_packed_halves(64, 64);
    const double lfl = 2.0 * nf * 9 * nf * px, lby = 2.0 * px * 2 * nf + 2.0 * 9 * nf * nf;
    uint16_t *HA = p->HA, *HB = p->HB;
    go(K_F16_PACK, 0, px * (4.0 * (c.in_nc + s2dc) + 2.0 * 64), [&] {
      return tg_conv3x3_f16_pack_input(lr_curr, c.in_nc * hw, c.in_nc, p->S2D, s2dc * hw, s2dc, HB, n, h, w, st);
    });
    auto hconv = [&](int k, const uint16_t* xin, const uint16_t* res, uint16_t* y, int act) {
      go(K_F16_CONV, lfl, lby + (res ? 2.0 * px * nf : 0), [&] {
        return tg_conv3x3_f16_fwd(xin, p->HWT + k * wstep, p->HL[k].b, res, y, n, 64, 64, h, w, act, st);
      });
    };
    hconv(0, HB, nullptr, HA, TG_ACT_RELU);
    for (int b = 0; b < c.nb; ++b) {
      hconv(1 + 2 * b, HA, nullptr, HB, TG_ACT_RELU);
      hconv(2 + 2 * b, HB, HA, HA, TG_ACT_NONE);
    }
    go(K_F16_CONVT, lfl, 2.0 * px * nf + 4.0 * px * nf * 4 + 2.0 * 9 * nf * nf, [&] {
      return tg_convt3x3s2_f16_fwd(HA, p->HWT + nbody * wstep, p->HL[nbody].b, p->U1, (int64_t)nf * 4 * hw, n, 64, 64, h,
                                   w, TG_ACT_RELU, st);
    });
  }

  // ---- the HR stage (tecogan_nets.py:119-131) --------------------------------------------------------------------------
  // SRNet's first up-sampling layer as a launch of its own: A -> U1
  void up1_launch() {
    const tg_layer_weights lw = p->L[at.up1];
    go(K_CONVT, 2.0 * nf * 9 * nf * n * hw, 4.0 * n * hw * nf * 5.0, [&] {
      return tg_convt3x3s2_fwd(p->A, nf * hw, lw.w, lw.b, p->U1, nf * 4 * hw, n, nf, nf, h, w, TG_ACT_RELU, st);
    });
  }
  // fused: the last up-sampling layer in Z mode (U1 at 4x, A at 2x -> conv_out's tap planes), then the tail
  void hr_fused_stage(const Choices& ch, const float* lr_curr, float* hr_out, uint8_t* u8_out) {
    float* zbuf = s == 4 ? p->U2 : p->U1;          // the 64-channel tensor is never written: its space holds the planes
    const int zh = s * h / 2, zw = s * w / 2;      // input size of the last up-sampling layer
    const float* zin = s == 4 ? p->U1 : p->A;
    const tg_layer_weights lw_last = p->L[s == 4 ? at.up2 : at.up1], lw_out = p->L[at.out];
    if (dry && ch.z_two) p->st_launch[K_CONVT_Z] += 1;
    go(K_CONVT_Z, 2.0 * nf * 9 * nf * n * zh * zw + 2.0 * nf * 9 * c.out_nc * hpx,
       4.0 * n * zh * zw * nf + 4.0 * hpx * 9 * c.out_nc, [&] {
         if (ch.z_wino)
           return tg_convt3x3s2_z_wino_fwd(zin, (int64_t)nf * zh * zw, p->WA, lw_last.b, p->WZ, c.out_nc, zbuf,
                                           (int64_t)32 * s * s * hw, n, nf, nf, zh, zw, TG_ACT_RELU, -1, st);
         return tg_convt3x3s2_z_fwd(zin, (int64_t)nf * zh * zw, lw_last.w, lw_last.b, p->WZ, c.out_nc, zbuf,
                                    (int64_t)32 * s * s * hw, n, nf, nf, zh, zw, TG_ACT_RELU, st);
       });
    go(K_TAIL, 0, 4.0 * hpx * (9 * c.out_nc + c.out_nc), [&] {
      return tg_convout_tail(zbuf, (int64_t)32 * s * s * hw, c.out_nc, lw_out.b, lr_curr, c.up_mode, s, hr_out,
                             (int64_t)c.out_nc * s * s * hw, u8_out, n, s * h, s * w, st);
    });
  }
  // unfused: the second transposed conv at 4x, the output conv, and the quantise pass where that cannot emit the bytes itself
  void hr_unfused_stage(const float* lr_curr, float* hr_out, uint8_t* u8_out) {
    const float* top = p->U1;
    if (s == 4) {
      const tg_layer_weights lw_up2 = p->L[at.up2];
      go(K_CONVT, 2.0 * nf * 9 * nf * n * 4 * hw, 4.0 * n * 4 * hw * nf * 5.0, [&] {
        return tg_convt3x3s2_fwd(p->U1, nf * 4 * hw, lw_up2.w, lw_up2.b, p->U2, nf * 16 * hw, n, nf, nf, 2 * h, 2 * w,
                                 TG_ACT_RELU, st);
      });
      top = p->U2;
    }
    const tg_layer_weights lw_out = p->L[at.out];
    const bool u8_fused = !dry && u8_out && tg_conv3x3_small_can_fuse_u8(top, (int64_t)nf * s * s * hw, hr_out,
                                                                         (int64_t)c.out_nc * s * s * hw, n, nf, s * h, s * w);
    go(K_SMALL, 2.0 * nf * 9 * c.out_nc * hpx, 4.0 * hpx * (nf + c.out_nc), [&] {
      return tg_conv3x3_small_fwd_u8(top, (int64_t)nf * s * s * hw, lw_out.w, lw_out.b, lr_curr, c.up_mode, s, hr_out,
                                     (int64_t)c.out_nc * s * s * hw, u8_fused ? u8_out : nullptr, n, nf, c.out_nc,
                                     s * h, s * w, TG_ACT_NONE, st);
    });
    if ((u8_out && !u8_fused) || dry)      // (w % 4 != 0, unaligned planes)
      go(K_QUANT, 0, 5.0 * c.out_nc * s * s * hw, [&] { return tg_quantize_u8_hwc(hr_out, u8_out, c.out_nc, s * h, s * w, st); });
  }
};

// One frame: phase 1 writes the flow slot, phase 2 reads it (or flow_ext, the flow of its frame from another plan's
// batched FNet pass).  dry: nothing is launched or dereferenced, the launches are accounted (account below).
static int emit_frame(tg_frnet_plan* p, const float* lr_curr, const float* lr_prev, const float* hr_prev, float* hr_out,
                      uint8_t* u8_out, tg_stream_t st, unsigned mask, bool dry, int phases = 3, int slot = 0,
                      const float* flow_ext = nullptr) {
  if (!dry && (phases & 2) && mask == 0xFFFFFFFFu) chain_rearm_tick(p, st);
  const Choices ch = choose(p, one_launch_off(p));
  Emit em{p, st, mask, dry, phases};
  const float* flow = em.fnet_stage(lr_curr, lr_prev, flow_ext ? const_cast<float*>(flow_ext) : (slot ? p->FLOW2 : p->FLOW));
  em.begin_phase(2);
  em.prepare_packs(ch);
  em.warp_stage(flow, hr_prev);
  if (ch.body == BODY_F16) em.body_f16(lr_curr);
  else if (ch.body == BODY_LAYERS) em.body_layers(lr_curr, 0, 1 + 2 * p->cfg.nb);
  else em.body_one_launch(ch, lr_curr);
  // a launch of its own unless it rode on the body or, at 2x, is the fused stage's Z layer itself
  if (!ch.ct_fold && !(ch.hr_fused && p->cfg.scale == 2)) em.up1_launch();
  if (ch.hr_fused) em.hr_fused_stage(ch, lr_curr, hr_out, u8_out);
  else em.hr_unfused_stage(lr_curr, hr_out, u8_out);
  return em.rc;
}

// dry run: per-kernel-class launch counts, algorithmic flops and bytes of one frame
static void account(tg_frnet_plan* p) {
  for (int k = 0; k < K_COUNT; ++k) { p->st_launch[k] = 0; p->st_flops[k] = 0; p->st_bytes[k] = 0; }
  p->chain_layers = 0;
  static float dummy;      // (non-null pointers; nothing is dereferenced or launched)
  emit_frame(p, &dummy, &dummy, &dummy, &dummy, nullptr, nullptr, 0, true);
  p->launches = 0;
  for (int k = 0; k < K_COUNT; ++k) p->launches += p->st_launch[k];
  p->launches -= p->st_launch[K_QUANT];  // quantise only runs when a u8 output is requested
}

// ---- the C ABI ---------------------------------------------------------------------------------------------------------
// out_nc == in_nc: the frame is fed back as hr_prev (read as in_nc channels), and the output conv adds the up-sampled
// lr_curr, which the small-cout kernel and the tail index with out_nc channels per image (tecogan_nets.py:145, :250
// need the same) -- out_nc = 4 would read past lr_curr, out_nc < 3 the wrong image of a batch.
static int cfg_ok(const tg_frnet_cfg* c) {
  return c && c->in_nc == 3 && c->out_nc == c->in_nc && c->nf >= 1 && c->nf <= 64 && c->nb >= 0 &&
         (c->scale == 2 || c->scale == 4) && (c->up_mode == TG_UP_BICUBIC || c->up_mode == TG_UP_BILINEAR) &&
         c->n >= 1 && c->h >= 8 && c->w >= 8;
}

extern "C" size_t tg_frnet_workspace_floats(const tg_frnet_cfg* cfg) {
  size_t off[R_COUNT];
  return cfg_ok(cfg) ? carve(cfg, off) : 0;
}

extern "C" int tg_frnet_plan_create(const tg_frnet_cfg* cfg, const tg_layer_weights* layers,
                                    int n_layers, float* workspace, tg_frnet_plan** out) {
  TG_REQUIRE(cfg && layers && workspace && out, TG_E_ARG, "frnet_plan_create: null pointer");
  TG_REQUIRE(cfg_ok(cfg), TG_E_SHAPE,
             "frnet_plan_create: unsupported cfg (in_nc=3, out_nc=in_nc, nf<=64, scale 2|4, h,w>=8)");
  const LayerIndex at(cfg->nb, cfg->scale);
  TG_REQUIRE(n_layers == at.count, TG_E_ARG, "frnet_plan_create: %d layers given, %d expected", n_layers, at.count);
  for (int i = 0; i < n_layers; ++i)
    TG_REQUIRE(layers[i].w && layers[i].b, TG_E_ARG, "frnet_plan_create: layer %d null", i);
  tg_frnet_plan* p = new (std::nothrow) tg_frnet_plan();
  TG_REQUIRE(p, TG_E_ARG, "frnet_plan_create: out of host memory");
  p->cfg = *cfg; p->at = at;
  p->L.assign(layers, layers + n_layers);
  size_t off[R_COUNT];
  carve(cfg, off);
  auto region = [&](int r) { return workspace + off[r]; };
  p->A = region(R_A); p->B = region(R_B); p->FLOW = region(R_FLOW); p->S2D = region(R_S2D); p->U1 = region(R_U1);
  p->U2 = cfg->scale == 4 ? region(R_U2) : nullptr; p->PART = region(R_PART);
  p->FA = region(R_FA); p->FB = region(R_FB); p->FPART = region(R_FPART); p->FLOW2 = region(R_FLOW2);
  p->WZ = region(R_WZ_WA); p->WA = p->WZ + 2048;
  p->UPZ = region(R_UPZ); p->UPA = region(R_UPA);
  p->CHAINF = reinterpret_cast<int32_t*>(region(R_CHAINF)); p->RESWS = region(R_RESWS);
  if (!cfg->fnet_only) {
    void* hp = nullptr;
    if (hipHostMalloc(&hp, 64, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess && hp) {
      p->chain_err = static_cast<int32_t*>(hp);
      for (int i = 0; i < 16; ++i) p->chain_err[i] = 0;
    } else {
      (void)hipGetLastError();      // no fault channel -> no chained launch (per-layer launches are always safe)
    }
  }
  p->fh = cfg->h / 8 * 8; p->fw = cfg->w / 8 * 8;
  account(p);
  *out = p;
  return TG_OK;
}

extern "C" void tg_frnet_plan_destroy(tg_frnet_plan* plan) {
  if (!plan) return;
  // (a chained launch still in flight may yet add to the counter: the caller synchronises before
  // destroying a plan, as for the workspace it owns)
  if (plan->chain_err) (void)hipHostFree(plan->chain_err);
  if (plan->rearm_fence) (void)hipEventDestroy(plan->rearm_fence);
  delete plan;
}
extern "C" int tg_frnet_plan_launches(const tg_frnet_plan* plan) { return plan ? plan->launches : 0; }

// what the frame entry points check behind their pointers, and the fail-safe's report
static int frame_call_ok(tg_frnet_plan* p, const uint8_t* u8_out, bool phase2, const char* who) {
  TG_REQUIRE(!u8_out || plan_u8_ok(p), TG_E_ARG, "%s: u8 output needs n == 1 (or the fused HR stage)", who);
  TG_REQUIRE(!phase2 || !p->cfg.fnet_only, TG_E_ARG, "%s: the plan was created FNet-only", who);
  return chain_poll(p);
}

extern "C" int tg_frnet_step(tg_frnet_plan* p, const float* lr_curr, const float* lr_prev, const float* hr_prev,
                             float* hr_out, uint8_t* u8_out, tg_stream_t st) {
  return tg_frnet_step_masked(p, lr_curr, lr_prev, hr_prev, hr_out, u8_out, 0xFFFFFFFFu, st);
}

extern "C" int tg_frnet_step_masked(tg_frnet_plan* p, const float* lr_curr, const float* lr_prev, const float* hr_prev,
                                    float* hr_out, uint8_t* u8_out, unsigned kind_mask, tg_stream_t st) {
  TG_REQUIRE(p && lr_curr && lr_prev && hr_prev && hr_out, TG_E_ARG, "frnet_step: null pointer");
  if (int rc = frame_call_ok(p, u8_out, true, "frnet_step")) return rc;
  return emit_frame(p, lr_curr, lr_prev, hr_prev, hr_out, u8_out, st, kind_mask, false);
}

extern "C" float* tg_frnet_plan_flow(tg_frnet_plan* p, int flow_slot) {
  if (!p || (flow_slot != 0 && flow_slot != 1)) return nullptr;
  return flow_slot ? p->FLOW2 : p->FLOW;
}

extern "C" int tg_frnet_step_srnet(tg_frnet_plan* p, const float* lr_flow, const float* lr_curr, const float* hr_prev,
                                   float* hr_out, uint8_t* u8_out, tg_stream_t st) {
  TG_REQUIRE(p && lr_flow && lr_curr && hr_prev && hr_out, TG_E_ARG, "frnet_step_srnet: null pointer");
  if (int rc = frame_call_ok(p, u8_out, true, "frnet_step_srnet")) return rc;
  return emit_frame(p, lr_curr, nullptr, hr_prev, hr_out, u8_out, st, 0xFFFFFFFFu, false, 2, 0, lr_flow);
}

extern "C" int tg_frnet_step_phase(tg_frnet_plan* p, int phases, int flow_slot, const float* lr_curr, const float* lr_prev,
                                   const float* hr_prev, float* hr_out, uint8_t* u8_out, tg_stream_t st) {
  TG_REQUIRE(p && lr_curr, TG_E_ARG, "frnet_step_phase: null pointer");
  TG_REQUIRE(phases >= 1 && phases <= 3 && (flow_slot == 0 || flow_slot == 1), TG_E_ARG,
             "frnet_step_phase: phases=%d slot=%d", phases, flow_slot);
  TG_REQUIRE(!(phases & 1) || lr_prev, TG_E_ARG, "frnet_step_phase: phase 1 needs lr_prev");
  TG_REQUIRE(!(phases & 2) || (hr_prev && hr_out), TG_E_ARG, "frnet_step_phase: phase 2 needs hr_prev/hr_out");
  if (int rc = frame_call_ok(p, u8_out, (phases & 2) != 0, "frnet_step_phase")) return rc;
  return emit_frame(p, lr_curr, lr_prev, hr_prev, hr_out, u8_out, st, 0xFFFFFFFFu, false, phases, flow_slot);
}

// measurement helper: enqueue the masked launch list `reps` times from C (no host round
// trip per replay, so single-launch kernel classes are timed GPU-bound)
extern "C" int tg_frnet_replay(tg_frnet_plan* p, const float* lr_curr, const float* lr_prev, const float* hr_prev,
                               float* hr_out, unsigned kind_mask, int reps, tg_stream_t st) {
  TG_REQUIRE(p && lr_curr && lr_prev && hr_prev && hr_out && reps > 0 && !p->cfg.fnet_only, TG_E_ARG,
             "frnet_replay: bad argument");
  if (int rc = chain_poll(p)) return rc;
  for (int i = 0; i < reps; ++i)
    if (int rc = emit_frame(p, lr_curr, lr_prev, hr_prev, hr_out, nullptr, st, kind_mask, false)) return rc;
  return TG_OK;
}

extern "C" int tg_frnet_plan_chain_status(tg_frnet_plan* p, int* faults_total, int* chain_active) {
  TG_REQUIRE(p, TG_E_ARG, "frnet_plan_chain_status: null plan");
  const int rc = chain_poll(p);
  if (faults_total) *faults_total = p->chain_faults;
  if (chain_active) *chain_active = (p->chain_layers > 0 && !p->chain_disabled) ? 1 : 0;
  return rc;
}

extern "C" int tg_frnet_plan_set_chain_poll_limit(tg_frnet_plan* p, int poll_limit) {
  TG_REQUIRE(p, TG_E_ARG, "frnet_plan_set_chain_poll_limit: null plan");
  p->chain_poll_limit = poll_limit;
  return TG_OK;
}

extern "C" int tg_frnet_plan_set_chain_rearm(tg_frnet_plan* p, int first_after_frames) {
  TG_REQUIRE(p && first_after_frames >= 0, TG_E_ARG, "frnet_plan_set_chain_rearm: bad argument");
  p->rearm_first = first_after_frames;
  if (p->chain_disabled && p->rearm_wait == 0) p->rearm_wait = first_after_frames;
  return TG_OK;
}

extern "C" int tg_frnet_plan_hold_chain_rearm(tg_frnet_plan* p, int hold) {
  TG_REQUIRE(p, TG_E_ARG, "frnet_plan_hold_chain_rearm: null plan");
  p->rearm_hold = hold != 0;
  return TG_OK;
}

extern "C" int tg_frnet_plan_chain_rearms(const tg_frnet_plan* p, int* rearms, int* current_wait_frames) {
  TG_REQUIRE(p, TG_E_ARG, "frnet_plan_chain_rearms: null plan");
  if (rearms) *rearms = p->rearms;
  if (current_wait_frames) *current_wait_frames = p->rearm_wait;
  return TG_OK;
}

extern "C" size_t tg_frnet_f16_workspace_bytes(const tg_frnet_cfg* cfg) {
  if (!cfg_ok(cfg) || cfg->fnet_only || cfg->nf != 64) return 0;
  const size_t wbytes = (size_t)(2 + 2 * cfg->nb) * tg_conv3x3_f16_packed_halves(64, 64) * 2;
  const size_t abytes = (size_t)tg_conv3x3_f16_act_halves(cfg->n, cfg->h, cfg->w) * 2;
  return align64(wbytes) + 2 * align64(abytes);
}

extern "C" int tg_frnet_plan_set_precision(tg_frnet_plan* p, int precision, const tg_layer_weights* plain,
                                           int n_plain, void* workspace) {
  TG_REQUIRE(p, TG_E_ARG, "frnet_plan_set_precision: null plan");
  TG_REQUIRE(precision == TG_PREC_F32 || precision == TG_PREC_F16, TG_E_ARG,
             "frnet_plan_set_precision: precision %d (TG_PREC_F32 | TG_PREC_F16)", precision);
  if (precision == TG_PREC_F16) {
    const tg_frnet_cfg& c = p->cfg;
    TG_REQUIRE(!c.fnet_only, TG_E_ARG, "frnet_plan_set_precision: an FNet-only plan has no SRNet body");
    TG_REQUIRE(c.nf == 64 && tg_conv3x3_f16_supported(c.n, 64, 64, c.h, c.w), TG_E_ARG,
               "frnet_plan_set_precision: the fp16 body needs nf = 64 (nf = %d)", c.nf);
    TG_REQUIRE(plain && n_plain == 2 + 2 * c.nb, TG_E_ARG, "frnet_plan_set_precision: %d plain layers given, %d expected",
               n_plain, 2 + 2 * c.nb);
    for (int i = 0; i < n_plain; ++i)
      TG_REQUIRE(plain[i].w && plain[i].b, TG_E_ARG, "frnet_plan_set_precision: plain layer %d null", i);
    TG_REQUIRE(workspace && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0, TG_E_ARG,
               "frnet_plan_set_precision: workspace null or not 16-byte aligned");
    p->HL.assign(plain, plain + n_plain);
    const size_t wbytes = align64((size_t)n_plain * tg_conv3x3_f16_packed_halves(64, 64) * 2);
    const size_t abytes = align64((size_t)tg_conv3x3_f16_act_halves(c.n, c.h, c.w) * 2);
    unsigned char* base = static_cast<unsigned char*>(workspace);
    p->HWT = reinterpret_cast<uint16_t*>(base);
    p->HA = reinterpret_cast<uint16_t*>(base + wbytes);
    p->HB = reinterpret_cast<uint16_t*>(base + wbytes + abytes);
    p->f16_ready = false;
  }
  p->f16 = precision == TG_PREC_F16;
  // back in fp32 the one-launch bodies start from zeroed flags / exchange buffers, as after plan_create
  p->res_ready = false; p->chain_ready = false;
  account(p);
  return TG_OK;
}

extern "C" int tg_frnet_plan_precision(const tg_frnet_plan* p) { return p && p->f16 ? TG_PREC_F16 : TG_PREC_F32; }
extern "C" int tg_frnet_plan_kinds(void) { return K_COUNT; }

extern "C" const char* tg_frnet_kind_name(int kind) {
  static const char* names[K_COUNT] = {
      "conv3x3_mfma_kernel<2,2,1>", "conv3x3_mfma_kernel<4,1,2>", "conv3x3_mfma_kernel<4,1,1>",
      "convt3x3s2_mfma_kernel",      "conv3x3_small_kernel",       "flowup_warp_s2d_kernel",
      "maxpool2_kernel",             "upsample_kernel",            "quantize_u8_hwc_kernel",
      "splitk_finalize_kernel",      "conv3x3_mfma_kernel<1,2,1,KS=2>",
      "convt3x3s2_mfma_kernel<Z>",   "convout_tail_kernel",        "conv3x3_oneshot_kernel",
      "conv3x3_wino_kernel",         "conv3x3_wino_chain_kernel",  "conv3x3_wino_resident_kernel",
      "pack_input_f16_kernel",       "conv3x3_f16_kernel<false>",  "conv3x3_f16_kernel<true>"};
  return (kind >= 0 && kind < K_COUNT) ? names[kind] : "?";
}

extern "C" int tg_frnet_plan_kind_stats(const tg_frnet_plan* p, int kind, int* launches, double* flops, double* bytes) {
  TG_REQUIRE(p && kind >= 0 && kind < K_COUNT, TG_E_ARG, "plan_kind_stats: bad argument");
  if (launches) *launches = p->st_launch[kind];
  if (flops) *flops = p->st_flops[kind];
  if (bytes) *bytes = p->st_bytes[kind];
  return TG_OK;
}
