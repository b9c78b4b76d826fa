// SRNet's conv_in + residual-block convs (tecogan_nets.py:85-100, 108-116, 141-143) of ONE
// 134x320-class frame as ONE launch of PERSISTENT, LDS-RESIDENT workgroups (round 4).
//
// Why: the per-layer Winograd kernel (tg_conv3x3_wino.hip) spends ~10 of its ~23 us per layer on
// cost every one of its 670 co-resident workgroups pays in lockstep -- launch, first loads of the
// 11 MB input, the 11 MB of stores nothing overlaps, drain.  A 64-channel
// 134x320 activation is 11 MB = 43 KB per CU: it FITS in the LDS of the 256 CUs.  So here
//   * one workgroup per CU owns a block of 8 x 24 pixels (4 x 12 Winograd tiles = three MFMA groups
//     of 16 tiles) for ALL the layers; the block (+ a one-pixel ring) of the current and of the next
//     layer live in two LDS buffers of 64 x 10 x 28 floats (ping-pong; the residual input of a
//     ResidualBlock is what the destination buffer still holds: x -> conv1 -> other buffer ->
//     conv2 -> += x in place);
//   * between two layers only the block's outermost ring of pixels travels: 64 pixels x 64 channels
//     = 16 KB per workgroup through an exchange buffer in global memory (agent-scope 16-byte stores,
//     one monotonic flag per workgroup, 16-byte agent-scope loads of the <= 8 neighbours' rings)
//     instead of 11 MB written + 11 MB read per layer;
//   * 12 waves = 3 tile groups x 4 output-channel blocks of 16 (the three waves that share a SIMD
//     share a weight slice, so their loads hit L1); a wave builds its MFMA B operand (the
//     transformed input window B^T d B) in REGISTERS straight from the resident block -- no V tensor
//     in LDS, no barrier inside the K loop (the per-layer kernel has 8);
//   * same arithmetic in the same order as conv3x3_wino_kernel (same packed U, K ascending, same
//     transform / inverse-transform expressions): results are BIT-IDENTICAL to the per-layer
//     launches (tests/test_hip_parity.py::test_wino_resident_*).
// Forward progress needs every workgroup resident at once (neighbours wait for each other in both
// directions): the launcher refuses grids above the device's CU count minus a margin, and the kernel
// is FAIL-SAFE like the other chained launches (poll limit -> fault counter in pinned host memory
// -> the plan reports TG_E_HIP and runs one launch per layer for good).
//
// TG_FILE_FLAGS: -fno-slp-vectorize
// (build.sh passes this line's flags to hipcc for THIS file.  With the K loop one straight-line block the SLP
// vectorizer pairs the transform's adds into v_pk_add_f32 and pays for it with ~12 v_mov_b32 per K step -- every VALU
// instruction adds to the fp32-MFMA time on this pipe: 21.2 vs 18.9 us per layer, round 5.)
#include <type_traits>

#include "tg_common.h"
#include "tg_launch.h"

// ---- the one build switch.  WR_UASM = 1 is what ships: hand-written weight requests + exact vmcnt waits (round 5).
// WR_UASM = 0 is the round-4 form of the same kernel -- compiler-visible weight loads behind a branch, the compiler's own
// waits -- and exists as the reference the hand-written waits are checked against: tests/test_hip_soak.py rebuilds this
// file with it and requires bit-identical results.  It needs -DTG_LAB=1, which csrc/build.sh refuses for the in-tree
// library.  (The variants that lost their A/B -- wave priorities, three weight blocks in flight, inline-asm window reads,
// the packed input transform, the ablation bits -- are written up in EXPERIMENTS.md and live in git history.) ----
#ifndef WR_UASM
#define WR_UASM 1
#endif
#if !TG_LAB && WR_UASM != 1
#error "tg_conv3x3_wino_res.hip: a lab switch is set without -DTG_LAB=1 (the in-tree library ships the defaults only)"
#endif

namespace tg {

int wres_lab_bits() { return (WR_UASM != 1 ? 32 : 0) | (TG_LAB ? 1024 : 0); }    // tg_build_info(): 0 in the shipped library

constexpr int WR_TH = 4, WR_TW = 12;             // Winograd tiles per block
constexpr int WR_BH = 2 * WR_TH, WR_BW = 2 * WR_TW;   // 8 x 24 pixels
constexpr int WR_RS = 28;                         // LDS row stride (floats): ring + 24 + ring + 2 pad
constexpr int WR_CS = 288;                        // channel stride: 10 rows x 28 = 280 -> 288 = 32 mod 64:
                                                  // the 32 lanes of a ds_read_b64 group (2 channels x 16 tiles) hit 64 distinct banks
constexpr int WR_NC = 64;                         // channels (nf)
constexpr int WR_THREADS = 768;                   // 12 waves: 3 per SIMD
constexpr int WR_MAXL = 24;
constexpr int WT_NP = 25;                         // the tail's products per tile and K step (WZ_NP of tg_convt3x3s2_wino.hip)
constexpr int WR_SLOTS = 64;                      // published ring pixels of a block: top 24, bottom 24, left 8, right 8
constexpr int WR_POLL_SLEEP = 2;                  // s_sleep units (64 cycles) between two polls of the ring
constexpr int WR_ACT_FLOATS = 2 * WR_NC * WR_CS;   // the two activation buffers: 147 456 bytes
constexpr int WR_BIAS_OFF = WR_ACT_FLOATS;          // [layer][64] biases (read once per launch)
constexpr int WR_SYNC_OFF = WR_BIAS_OFF + WR_MAXL * WR_NC;   // 16 bytes: arrival counter of the boundary waves
constexpr int WR_NRING = 2 * (WR_BW + 2) + 2 * WR_BH;   // 68 ring pixels: top 26, bottom 26, left 8, right 8
constexpr int WR_RING_TAB = 80;                   // ring table entries: a boundary thread's five pixels are pi, pi + 16, ... <= 79
constexpr int WR_RING_OFF = WR_SYNC_OFF + 4;      // [80] one word per ring pixel, filled once per launch (wres_ring_item)
constexpr size_t WR_LDS_BYTES = (size_t)(WR_RING_OFF + WR_RING_TAB) * sizeof(float);   // 153 936 of 163 840
static_assert(WR_RING_OFF % 4 == 0 && WR_NRING <= WR_RING_TAB && WR_LDS_BYTES <= 163840, "ring table placement");

// Ring pixel pi = 0..67 of block (bx, by) -- top row, bottom row, left column, right column of the block's one-pixel
// ring -- and where the hand-over finds it: the block that owns the pixel, the slot under which that block publishes
// it (top row 0.., bottom row WR_BW.., left column 2 WR_BW.., right column 2 WR_BW + WR_BH..: see `pub` in the kernel)
// and the pixel's place in the LDS block.  valid = 0: the pixel lies outside the image (it is never fetched and stays 0).
// A function of (h, w, block, pixel) only: the kernel tabulates it once per launch, the host exports it for the tests.
struct WResRingItem { int valid, owner, slot, lds; };
__host__ __device__ inline WResRingItem wres_ring_item(int h, int w, int nbx, int bx, int by, int pi) {
  int ry, rx;
  if (pi < WR_BW + 2) { ry = 0; rx = pi; }
  else if (pi < 2 * (WR_BW + 2)) { ry = WR_BH + 1; rx = pi - (WR_BW + 2); }
  else if (pi < 2 * (WR_BW + 2) + WR_BH) { ry = pi - 2 * (WR_BW + 2) + 1; rx = 0; }
  else { ry = pi - 2 * (WR_BW + 2) - WR_BH + 1; rx = WR_BW + 1; }
  const int gy = by * WR_BH - 1 + ry, gx = bx * WR_BW - 1 + rx;
  WResRingItem it{0, -1, -1, ry * WR_RS + rx};
  if (gy >= 0 && gy < h && gx >= 0 && gx < w) {
    const int sby = gy / WR_BH, sbx = gx / WR_BW;
    const int ly = gy - sby * WR_BH, lx = gx - sbx * WR_BW;
    // which of the owner's published rows / columns holds the pixel
    it.slot = ry == 0 ? WR_BW + lx : (ry == WR_BH + 1 ? lx : (rx == 0 ? 2 * WR_BW + WR_BH + ly : 2 * WR_BW + ly));
    it.owner = sby * nbx + sbx;
    it.valid = 1;
  }
  return it;
}

// Tile (ty * 12 + tx) of lane n = 0..15 of group g.  Group 2 holds INTERIOR tiles only (rows 1-2, columns
// 1..10: their 4x4 windows never touch the ring), so its four waves start the next layer right behind the
// workgroup barrier while the waves of groups 0 and 1 wait for the neighbours' rings.  Chosen (brute force)
// so that the 32 lanes of a ds_read_b64 group hit distinct bank pairs but for four two-way collisions.
__constant__ unsigned char WR_TILE[48] = {
    0, 1, 3, 4, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15, 24, 39,
    2, 8, 16, 23, 35, 36, 37, 38, 40, 41, 42, 43, 44, 45, 46, 47,
    17, 18, 19, 20, 21, 22, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34};


struct WResLayer {
  const float* u;      // tg_pack_conv3x3_wino form
  const float* bias;
  int act;
  int res;             // + the destination buffer's old content (residual input) after the activation
  int nks;             // K steps of 4 input channels, an even number (2 * ceil(cin / 8): the K loop walks in pairs)
  int pad;
};
struct WResArgs {
  WResLayer L[WR_MAXL];
  const float* x;      // first layer's input, channels [0, c1)
  const float* x2;     // channels [c1, cin0) or null
  float* y;            // last layer's output (64 x h x w)
  float* xbuf;         // exchange: [parity 2][block][slot 64][channel pair 32]{value, tag, value, tag}
  int* err;            // fault counter (pinned host memory or device memory)
  unsigned base;       // tag of layer l of this launch = base + l + 1 (strictly increasing over launches)
  int poll_limit;
  int nlayer, h, w, nbx, nby, c1, cin0;
  // optional tail: ConvTranspose2d(64, 64, 3, 2, 1, 1) + act of the last layer's output (SRNet's first up-sampling
  // layer, tecogan_nets.py:119-126) on the resident blocks; ct_u == null: the last layer's output goes to y
  const float* ct_u;   // tg_conv3x3_wino_resident_ct_pack form
  const float* ct_bias;
  float* ct_y;         // (64, 2h, 2w)
  int ct_act;
};

__global__ __launch_bounds__(WR_THREADS, 3) void conv3x3_wino_resident_kernel(WResArgs a) {
  extern __shared__ __attribute__((aligned(16))) float s_act[];    // [2][64][WR_CS]
  const int t = threadIdx.x, l = t & 63;
  const int wv = __builtin_amdgcn_readfirstlane(t >> 6);
  const int q = wv & 3;                       // output channels [16q, 16q + 16); waves q, q+4, q+8 share a SIMD and a weight slice
  const int g = wv >> 2;                      // tile group
  const int wg = blockIdx.x;
  const int bx = __builtin_amdgcn_readfirstlane(wg % a.nbx), by = __builtin_amdgcn_readfirstlane(wg / a.nbx);
  const int X0 = bx * WR_BW, Y0 = by * WR_BH;
  const int hw = a.h * a.w;
  const int nwg = a.nbx * a.nby;

  // ---- zero both buffers (rings at the image border and pixels outside the image stay 0) ----
  {
    f32x4* z = reinterpret_cast<f32x4*>(s_act);
    for (int i = t; i < WR_ACT_FLOATS / 4; i += WR_THREADS) z[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int i = t; i < a.nlayer * WR_NC; i += WR_THREADS) s_act[WR_BIAS_OFF + i] = a.L[i >> 6].bias[i & 63];
    if (t == 0) *reinterpret_cast<unsigned*>(s_act + WR_SYNC_OFF) = 0u;
    // the ring table: (owner block * 64 + slot + 1) << 16 | LDS offset of the pixel; high half 0 = nothing to fetch
    // (a pixel outside the image, an entry past the ring).  owner * 64 + slot + 1 <= 2^16: at most 1023 blocks, and
    // the launcher admits one per CU.  The hand-over of every layer decodes it instead of deriving it again.
    if (t < WR_RING_TAB) {
      const WResRingItem it = wres_ring_item(a.h, a.w, a.nbx, bx, by, t);
      reinterpret_cast<unsigned*>(s_act + WR_RING_OFF)[t] =
          t < WR_NRING && it.valid ? (unsigned)(it.owner * WR_SLOTS + it.slot + 1) << 16 | (unsigned)it.lds : 0u;
    }
  }
  unsigned* const s_cnt = reinterpret_cast<unsigned*>(s_act + WR_SYNC_OFF);
  __syncthreads();
  // ---- first layer's input block (+ ring) from global memory into buffer 0 ---------------
  // (bounds-checked buffer loads: zero padding, and the channels of the other source tensor, read 0;
  // every load of a batch is in flight before the first LDS store)
  {
    constexpr int WIN = (WR_BH + 2) * (WR_BW + 2);       // 260 pixels per channel
    const int total = a.cin0 * WIN;
    const __amdgpu_buffer_rsrc_t r1 = TG_BUF_RSRC(a.x, (unsigned)a.c1 * hw * 4u);
    const __amdgpu_buffer_rsrc_t r2 = TG_BUF_RSRC(a.x2 ? a.x2 : a.x, a.x2 ? (unsigned)(a.cin0 - a.c1) * hw * 4u : 0u);
    constexpr int BATCH = 11;
    for (int e0 = 0; e0 < total; e0 += BATCH * WR_THREADS) {
      float v[BATCH];
      int lo[BATCH];
#pragma unroll
      for (int k = 0; k < BATCH; ++k) {
        const int e = e0 + k * WR_THREADS + t;
        const int ic = e / WIN, rem = e - ic * WIN, r = rem / (WR_BW + 2), c = rem - r * (WR_BW + 2);
        const int gy = Y0 - 1 + r, gx = X0 - 1 + c;
        const bool in = e < total && gy >= 0 && gy < a.h && gx >= 0 && gx < a.w;
        const unsigned px = (unsigned)(gy * a.w + gx) * 4u;
        const unsigned o1 = (in && ic < a.c1) ? (unsigned)ic * hw * 4u + px : BUF_OOB;
        const unsigned o2 = (in && ic >= a.c1) ? (unsigned)(ic - a.c1) * hw * 4u + px : BUF_OOB;
        const float v1 = buf_ld<float>(r1, o1);
        const float v2 = buf_ld<float>(r2, o2);
        v[k] = ic < a.c1 ? v1 : v2;
        lo[k] = e < total ? ic * WR_CS + r * WR_RS + c : -1;
      }
#pragma unroll
      for (int k = 0; k < BATCH; ++k)
        if (lo[k] >= 0) s_act[lo[k]] = v[k];
    }
  }
  __syncthreads();

  // ---- per-lane geometry ---------------------------------------------------------------------
  const int T = WR_TILE[16 * g + (l & 15)];   // tile of the block (row-major 4 x 12)
  const int ty = T / WR_TW, tx = T - ty * WR_TW;
  const bool interior = g == 2;               // wave-uniform
  const int kk = l >> 4;                      // K index inside a K step (B operand) / output-channel quad (D)
  const int rb = kk * WR_CS + (2 * ty) * WR_RS + 2 * tx;        // window origin in the resident block (floats)
  const int oc_base = 16 * q + 4 * kk;
  const int wb = oc_base * WR_CS + (2 * ty + 1) * WR_RS + 2 * tx + 1;   // own 2x2 pixels, channel oc_base
  const int gy0 = Y0 + 2 * ty, gx0 = X0 + 2 * tx;               // image position of the tile
  const bool live = gy0 < a.h && gx0 < a.w;                     // h, w even: a tile is inside or outside as a whole
  const bool e_top = ty == 0, e_bot = ty == WR_TH - 1, e_lft = tx == 0, e_rgt = tx == WR_TW - 1;
  const __amdgpu_buffer_rsrc_t rxb = TG_BUF_RSRC(a.xbuf, (unsigned)(2u * nwg * WR_SLOTS * WR_NC * 8u));

  const size_t ulane = (size_t)(q * 4) * 64 + l;               // this lane's 16 bytes inside a K step's block
  constexpr size_t USTEP = (size_t)4 * 4 * 64;                  // f32x4 per K step (64 output channels)
  // The weight prefetch (round 5).  Two things kept a K step from ever running ahead of its weights:
  //  * a prefetch behind `if (ks < nks)` makes the compiler's s_waitcnt insertion merge the two paths at the join and
  //    assume the FEWER loads in flight: every K step waited `vmcnt(3..0)`, i.e. for the block requested a moment ago
  //    as well as for its own;
  //  * branch-free (past the last K step the last block is requested again: an L1 hit, never used) the same pass
  //    still emitted `vmcnt(0)` in this loop nest.
  // So the loads and their waits are written out (WR_UASM): the compiler does not see these loads, the waits carry the
  // exact counts -- a block's four loads are always followed by the four loads of the other block before it is used,
  // so `vmcnt(7..4)` releases it (at a layer's first K steps more has been issued in between: the wait is then merely
  // stronger than needed).  The compiler's own waits (ring, stores) count only its own operations and can only be
  // stronger than needed as well.  The stream of blocks runs ACROSS the layers: the last two K steps of a layer
  // request the first two blocks of the next one (they arrive under the epilogue and the hand-over), so exactly two
  // blocks are in flight at every point of the launch and the epilogue issues no request of its own.
  // Because the compiler cannot see these loads, csrc/build.sh FAILS the build if this kernel ever reports scratch or
  // spilled registers.
  [[maybe_unused]] const f32x4* un = nullptr;   // the next layer's blocks (the K loop runs on into them; WR_UASM only)
#if WR_UASM
  auto load_u = [&](const f32x4* ub, int ks, int nks, f32x4 (&u)[4]) {
    if (ks >= nks) { ub = un; ks -= nks; }      // uniform: a scalar select, no branch
    const f32x4* p = ub + (size_t)ks * USTEP;
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(u[0]) : "v"(p));
    asm volatile("global_load_dwordx4 %0, %1, off offset:1024" : "=v"(u[1]) : "v"(p));
    asm volatile("global_load_dwordx4 %0, %1, off offset:2048" : "=v"(u[2]) : "v"(p));
    asm volatile("global_load_dwordx4 %0, %1, off offset:3072" : "=v"(u[3]) : "v"(p));
  };
  // the block `u` was requested one block ago (see above): release it quarter by quarter
  auto wait_u = [&](f32x4 (&u)[4]) {
    asm volatile("s_waitcnt vmcnt(7)" : "+v"(u[0]));
    asm volatile("s_waitcnt vmcnt(6)" : "+v"(u[1]));
    asm volatile("s_waitcnt vmcnt(5)" : "+v"(u[2]));
    asm volatile("s_waitcnt vmcnt(4)" : "+v"(u[3]));
  };
  // Behind the K loop two blocks nobody uses are still in flight (the requests of the last two K steps): the
  // compiler takes their registers for dead and would hand them to the next instruction -- a landing load then
  // overwrites, say, the address of the epilogue's first request (a memory fault, found on the GPU).  The drain keeps
  // the eight registers allocated until every load has landed.
  auto drain_u = [&](f32x4 (&ua)[4], f32x4 (&ub_)[4]) {
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(ua[0]), "+v"(ua[1]), "+v"(ua[2]), "+v"(ua[3]),
                                        "+v"(ub_[0]), "+v"(ub_[1]), "+v"(ub_[2]), "+v"(ub_[3]));
  };
#else   // the cross-check form: plain loads, nothing requested past a layer's last K step, the compiler's waits
  auto load_u = [&](const f32x4* ub, int ks, int nks, f32x4 (&u)[4]) {
    if (ks >= nks) return;
    const f32x4* p = ub + (size_t)ks * USTEP;
    u[0] = p[0]; u[1] = p[64]; u[2] = p[128]; u[3] = p[192];
  };
  auto wait_u = [&](f32x4 (&)[4]) {};
  auto drain_u = [&](f32x4 (&)[4], f32x4 (&)[4]) {};
#endif

  f32x4 u0[4], u1[4];
  {
    const f32x4* ub = reinterpret_cast<const f32x4*>(a.L[0].u) + ulane;
    load_u(ub, 0, a.L[0].nks, u0);
    load_u(ub, 1, a.L[0].nks, u1);
  }

  const bool fold = a.ct_u != nullptr;        // launch-uniform
  for (int L = 0; L < a.nlayer; ++L) {
    const WResLayer& lay = a.L[L];
    const float* src = s_act + (L & 1) * (WR_NC * WR_CS);
    float* dst = s_act + ((L & 1) ^ 1) * (WR_NC * WR_CS);
    const f32x4* ub = reinterpret_cast<const f32x4*>(lay.u) + ulane;
    const int nks = lay.nks;
    // (behind the last layer its own first blocks are requested once more; drain_u retires them)
    un = reinterpret_cast<const f32x4*>(a.L[L + 1 < a.nlayer ? L + 1 : L].u) + ulane;

    f32x4 acc[16];
#pragma unroll
    for (int p = 0; p < 16; ++p) acc[p] = f32x4{0.f, 0.f, 0.f, 0.f};

    // the 4 x 4 window of channel 4 ks + kk at this lane's tile (the compiler merges the reads into ds_read2_b64)
    auto win_load = [&](int ks, float (&d)[4][4]) {
      const float* sp = src + rb + ks * (4 * WR_CS);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float2 p0 = *reinterpret_cast<const float2*>(sp + r * WR_RS);
        const float2 p1 = *reinterpret_cast<const float2*>(sp + r * WR_RS + 2);
        d[r][0] = p0.x; d[r][1] = p0.y; d[r][2] = p1.x; d[r][3] = p1.y;
      }
    };
    // one K step: window -> B^T d B in registers -> 16 MFMAs.  (fp32 MFMAs and VALU
    // instructions of the waves of a SIMD do NOT overlap on gfx950 -- tools/valu_lab.hip: 16 MFMAs + 32
    // adds take exactly the sum of both -- so the order inside a step matters little; a burst form with
    // the next window prefetched measured slower: 24.4 vs 21.5 us per layer, it costs registers.)
    auto kcompute = [&](const float (&d)[4][4], f32x4 (&u)[4]) {
      wait_u(u);
      f32x4 bq[4];
      float qa[4], qb[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) { qa[c] = d[0][c] - d[2][c]; qb[c] = d[1][c] + d[2][c]; }
      bq[0] = f32x4{qa[0] - qa[2], qa[1] + qa[2], qa[2] - qa[1], qa[1] - qa[3]};
      bq[1] = f32x4{qb[0] - qb[2], qb[1] + qb[2], qb[2] - qb[1], qb[1] - qb[3]};
#pragma unroll
      for (int c = 0; c < 4; ++c) { qa[c] = d[2][c] - d[1][c]; qb[c] = d[1][c] - d[3][c]; }
      bq[2] = f32x4{qa[0] - qa[2], qa[1] + qa[2], qa[2] - qa[1], qa[1] - qa[3]};
      bq[3] = f32x4{qb[0] - qb[2], qb[1] + qb[2], qb[2] - qb[1], qb[1] - qb[3]};
#pragma unroll
      for (int p = 0; p < 16; ++p)
        acc[p] = __builtin_amdgcn_mfma_f32_16x16x4f32(u[p >> 2][p & 3], bq[p >> 2][p & 3], acc[p], 0, 0, 0);
    };

    {   // window of K step ks + 1 in flight under the MFMAs of K step ks (the LDS latency of a K step is otherwise
        // exposed at its head: a wave that is alone on its SIMD -- the interior waves during the hand-over -- idles there)
      float dA[4][4], dB[4][4];
      win_load(0, dA);
      for (int ks = 0; ks < nks; ks += 2) {
        win_load(ks + 1, dB);
        __builtin_amdgcn_sched_barrier(0);      // (the scheduler otherwise sinks the reads to the end of the K step)
        kcompute(dA, u0);
        __builtin_amdgcn_sched_barrier(0);
        load_u(ub, ks + 2, nks, u0);
        win_load(ks + 2 < nks ? ks + 2 : ks, dA);
        __builtin_amdgcn_sched_barrier(0);
        kcompute(dB, u1);
        __builtin_amdgcn_sched_barrier(0);
        load_u(ub, ks + 3, nks, u1);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    // ---- inverse transform A^T m A, bias / activation / residual -----------------------------
    const bool last = L + 1 == a.nlayer && !fold;   // with the transposed-conv tail the last layer hands over like any other
    const float slope = act_slope(lay.act);
    float bz[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) bz[r] = s_act[WR_BIAS_OFF + L * WR_NC + oc_base + r];
    float v[4][2][2];                         // [channel r][row i][column j]
    // The activation is the generic form, 2 VALU per output (round 6): max(x, slope * x) = x >= 0 ? x : x * slope for
    // every slope in [0, 1] (ReLU 0, LeakyReLU 0.2, none 1), without a conditional move (v_cndmask_b32: ~23 cycles per
    // wave instruction on gfx950, tools/valu_lab.hip) -- the round-4 form max(x, 0) + slope * min(x, 0) was 3; on this
    // SIMD VALU time adds to the matrix time.  (Instantiations per activation -- ReLU as one v_max, nothing at all for
    // act none -- spill: 165 of 168 registers are taken, and this kernel must not spill: csrc/build.sh.)
    auto epilogue = [&](auto has_res) {
      constexpr bool RES = decltype(has_res)::value;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float sr[2][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          sr[0][j] = (acc[0 + j][r] + acc[4 + j][r]) + acc[8 + j][r];
          sr[1][j] = (acc[4 + j][r] - acc[8 + j][r]) - acc[12 + j][r];
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          float v0 = ((sr[i][0] + sr[i][1]) + sr[i][2]) + bz[r];
          float v1 = ((sr[i][1] - sr[i][2]) - sr[i][3]) + bz[r];
          v0 = __builtin_fmaxf(v0, slope * v0);
          v1 = __builtin_fmaxf(v1, slope * v1);
          if constexpr (RES) {                // the residual input: what the destination buffer still holds
            v0 += dst[wb + r * WR_CS + i * WR_RS];
            v1 += dst[wb + r * WR_CS + i * WR_RS + 1];
          }
          v[r][i][0] = v0; v[r][i][1] = v1;
        }
      }
    };
    if (lay.res) epilogue(std::true_type{}); else epilogue(std::false_type{});      // layer-uniform
#if !WR_UASM
    {   // the next layer's first weights travel under the hand-over (WR_UASM: the K loop has requested them already)
      const int Ln = L + 1 < a.nlayer ? L + 1 : L;
      const f32x4* un2 = reinterpret_cast<const f32x4*>(a.L[Ln].u) + ulane;
      load_u(un2, 0, a.L[Ln].nks, u0);
      load_u(un2, 1, a.L[Ln].nks, u1);
    }
#endif
    if (live) {
      if (last) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int i = 0; i < 2; ++i)
            *reinterpret_cast<float2*>(a.y + (size_t)(oc_base + r) * hw + (size_t)(gy0 + i) * a.w + gx0) =
                make_float2(v[r][i][0], v[r][i][1]);
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            dst[wb + r * WR_CS + i * WR_RS] = v[r][i][0];
            dst[wb + r * WR_CS + i * WR_RS + 1] = v[r][i][1];
          }
        // publish the block's outermost pixels as SELF-VALIDATING granules: {value, tag} pairs, two pairs
        // (channels c, c + 1) per 16-byte agent-scope store; tag = base + layer + 1 is unique per launch and
        // layer, so the reader needs no flag and the writer no acknowledgement (RCCL's LL idea; a 16-byte
        // sc1 store is observed untorn on gfx950).  Slot pixel-major: [slot 64][channel pair 32][4 dwords].
        const unsigned tag = a.base + (unsigned)(L + 1);
        const unsigned pb = ((unsigned)((L & 1) * nwg + wg) * WR_SLOTS * (WR_NC / 2) + (unsigned)(oc_base >> 1)) * 16u;
        auto pub = [&](int slot, int i, int j) {
          // (names the argument block so that [&] captures it: with no closure holding its address the compiler reads the
          // arguments in another order and commutes some thirty integer operands of the loader and of the ring geometry --
          // same results, but not the instruction stream every number in EXPERIMENTS.md was measured on)
          (void)a;
          const u32x4 d0 = {__builtin_bit_cast(unsigned, v[0][i][j]), tag, __builtin_bit_cast(unsigned, v[1][i][j]), tag};
          const u32x4 d1 = {__builtin_bit_cast(unsigned, v[2][i][j]), tag, __builtin_bit_cast(unsigned, v[3][i][j]), tag};
          const unsigned o = pb + (unsigned)slot * (WR_NC / 2 * 16u);
          buf_st<BUF_SC1>(d0, rxb, o);
          buf_st<BUF_SC1>(d1, rxb, o + 16u);
        };
        if (e_top) { pub(2 * tx, 0, 0); pub(2 * tx + 1, 0, 1); }
        if (e_bot) { pub(WR_BW + 2 * tx, 1, 0); pub(WR_BW + 2 * tx + 1, 1, 1); }
        if (e_lft) { pub(2 * WR_BW + 2 * ty, 0, 0); pub(2 * WR_BW + 2 * ty + 1, 1, 0); }
        if (e_rgt) { pub(2 * WR_BW + WR_BH + 2 * ty, 0, 1); pub(2 * WR_BW + WR_BH + 2 * ty + 1, 1, 1); }
      }
    }
    if (last) { drain_u(u0, u1); break; }

    // ---- hand-over -------------------------------------------------------------------------------
    // Every wave: the workgroup barrier (all of dst's own pixels are written, all reads of src are
    // done).  The four INTERIOR waves go straight on to the next layer: their windows never touch the
    // ring.  The eight BOUNDARY waves fetch the ring -- 68 pixels x 32 channel pairs, one 16-byte
    // agent-scope load per item, re-issued until both tags of the item carry this layer's value --
    // store it into dst and meet at an LDS arrival counter, while the interior waves already keep the
    // matrix pipe busy.
    __syncthreads();
    if (interior) continue;
    {
      constexpr int ITEMS = WR_NRING * (WR_NC / 2);                // 2176: 68 ring pixels x 32 channel pairs
      constexpr int NBT = 512;
      constexpr int PER_T = (ITEMS + NBT - 1) / NBT;               // 5 (4.25 on average)
      static_assert((NBT / 32) * (PER_T - 1) + NBT / 32 <= WR_RING_TAB, "every item of a boundary thread has a table entry");
      const unsigned target = a.base + (unsigned)(L + 1);
      unsigned off[PER_T];
      int ho[PER_T];
      unsigned pend = 0;
      int tt = t;
      asm volatile("" : "+v"(tt));            // keeps the decoded geometry out of the K loop's register budget (it would be hoisted and spilled)
      // Item tt + 512 k is (ring pixel (tt >> 5) + 16 k, channel pair tt & 31): the pixel's word of the ring table (the
      // 32 lanes of a half-wave read the same one), the thread's own channel pair, and the layer's parity -- one
      // wave-uniform term.  (Derived from (h, w, block, thread) in every hand-over it was ~230 VALU and
      // ~205 SALU instructions in front of the first ring load, 21 times per launch: EXPERIMENTS.md, "ring table".)
      const unsigned* tab = reinterpret_cast<const unsigned*>(s_act + WR_RING_OFF) + (tt >> 5);
      const unsigned c2 = (unsigned)tt & 31u;
      const unsigned obase = ((unsigned)((L & 1) * nwg) * WR_SLOTS - 1u) * (WR_NC / 2 * 16u) + c2 * 16u;   // (the entry's + 1)
      const int hbase = (int)(2u * c2) * WR_CS;
      unsigned po = 0u;                       // the probe: the thread's lowest pending item
      int ph = 0;
#pragma unroll
      for (int k = PER_T - 1; k >= 0; --k) {
        const unsigned e = tab[k * (NBT / 32)];
        off[k] = (e >> 16) * (WR_NC / 2 * 16u) + obase;
        ho[k] = hbase + (int)(e & 0xffffu);
        if (e >> 16) { pend |= 1u << k; po = off[k]; ph = ho[k]; }
      }
      // (plain scalars, initialised: with a vector array left undefined for items that are not pending the
      // compiler stored element 0 of an item into BOTH channels of its pair -- found on the GPU, round 4)
      unsigned q0[PER_T], q1[PER_T], q2[PER_T], q3[PER_T];
#pragma unroll
      for (int k = 0; k < PER_T; ++k) { q0[k] = 0u; q1[k] = 0u; q2[k] = 0u; q3[k] = 0u; }
      // While the neighbours are still computing, a thread polls ONE of its items (512 16-byte loads per
      // round and workgroup instead of 2176: the poll traffic queued in front of the interior waves'
      // weight loads was several times the weight traffic itself); once that one carries the tag the
      // rest is fetched in one go.  The probe is a loop of its own -- one load, two compares, two LDS stores -- so
      // that the usual hand-over (the probe carries the tag, so does everything fetched behind it) walks each item
      // once; the same polls, sleeps and limit as the one loop over a `want` mask this replaces.
      int polls = 0;
      bool fault = a.poll_limit < 0;
      // (The probe's granule, too, lives in plain initialised scalars and is stored BEHIND the loop: stored inside it,
      // from the loaded vector, the compiler wrote element 0 into both channels again -- the ISA showed
      // `ds_write_b32 v60, v50` twice -- and tests/test_hip_wres_handover.py failed at 16x48.)
      {
        unsigned p0 = 0u, p1 = 0u, p2 = 0u, p3 = 0u;
        bool got = false;
        while (pend != 0u && !got && !fault) {
          const u32x4 q = buf_ld<u32x4, BUF_SC1>(rxb, po);
          p0 = q[0]; p1 = q[1]; p2 = q[2]; p3 = q[3];
          got = p1 == target && p3 == target;
          if (!got) {
            __builtin_amdgcn_s_sleep(WR_POLL_SLEEP);
            fault = ++polls > a.poll_limit;
          }
        }
        if (got) {
          dst[ph] = __builtin_bit_cast(float, p0);
          dst[ph + WR_CS] = __builtin_bit_cast(float, p2);
          pend &= pend - 1u;                  // (the lowest pending item has arrived)
        }
      }
      while (pend != 0u && !fault) {
#pragma unroll
        for (int k = 0; k < PER_T; ++k)
          if (pend & (1u << k)) {
            const u32x4 q = buf_ld<u32x4, BUF_SC1>(rxb, off[k]);
            q0[k] = q[0]; q1[k] = q[1]; q2[k] = q[2]; q3[k] = q[3];
          }
        const unsigned want_mask = pend;
#pragma unroll
        for (int k = 0; k < PER_T; ++k)
          if ((want_mask & (1u << k)) && q1[k] == target && q3[k] == target) {
            dst[ho[k]] = __builtin_bit_cast(float, q0[k]);
            dst[ho[k] + WR_CS] = __builtin_bit_cast(float, q2[k]);
            pend &= ~(1u << k);
          }
        if (pend != 0u) {
          __builtin_amdgcn_s_sleep(WR_POLL_SLEEP);
          fault = ++polls > a.poll_limit;
        }
      }
      if (fault && pend != 0u) __hip_atomic_fetch_add(a.err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    // arrival counter of the eight boundary waves (monotonic over the launch): a wave's LDS stores are
    // ordered before its increment, so whoever reads the full count sees every ring pixel
    if (l == 0) __hip_atomic_fetch_add(s_cnt, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    {
      const unsigned want = 8u * (unsigned)(L + 1);
      while ((int)(__hip_atomic_load(s_cnt, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) - want) < 0)
        __builtin_amdgcn_s_sleep(1);
    }
  }
  if (!fold) return;
  drain_u(u0, u1);                            // (the requests behind the last layer's epilogue)

  // ---- tail: ConvTranspose2d(64, 64, 3, stride 2, pad 1, output_padding 1) + act on the resident block ------------
  //   out[2y + py][2x + px] = bias + sum_ic sum_taps in[y + dy][x + dx] W[ic][oc][ky][kx],
  //   py = 0: (dy 0, ky 1);  py = 1: (dy 0, ky 2), (dy 1, ky 0)   (the same along x; 9 taps over the 4 phases).
  // The wave keeps its (tile group, 16-channel block): MFMA column n = Winograd tile n of the group, and a lane's 3 x 3
  // window at its tile origin holds every operand of the tile's 2 x 2 input pixels (ya, xb) -- the operand set of
  // convt3x3s2_wino_z_kernel (tg_convt3x3s2_wino.hip), whose identity and conventions this tail follows: F(2,2) with
  // coefficients +-1 along each axis,
  //   data     c[i] = (d[i][0] - d[i][1], d[i][1], d[i][2] - d[i][1])   (the y-transform likewise over rows)
  //   weights  (g0, g1, g2) = (W[.2], W[.2] + W[.0], W[.0])             y(b) = m[b] + m[b + 1]
  // so the four phases need 4 + 6 + 6 + 9 = 25 products per tile and K step instead of the 36 of the direct form:
  //   p  0.. 3  phase (0,0): raw d[ya][xb]                       against W11                    p = 2 ya + xb
  //   p  4.. 9  phase (0,1): row ya, x-transform j               against (W12, W12 + W10, W10)  p = 4 + 3 ya + j
  //   p 10..15  phase (1,0): y-transform i, column xb            against (W21, W21 + W01, W01)  p = 10 + 2 i + xb
  //   p 16..24  phase (1,1): y-transform i, x-transform j        against G[i][j]                p = 16 + 3 i + j
  // G: rows (W2., W2. + W0., W0.), columns likewise, the centre the row sum of the column sums (convt_pack_wino_kernel).
  // 9 LDS reads, 16 subtractions, 7 weight sums (in registers, from the nine raw taps of the packed operand) and 25
  // MFMAs per K step, 25 accumulators.  Weights straight from L2 (two K steps in flight), output transform in the
  // epilogue (phase (1,1): rows first, as the Z kernel), output as 16-byte stores of 4 consecutive columns.
  __syncthreads();                            // the ring of the last layer is complete for EVERY wave
  {
    // (the tail's geometry is derived from an opaque copy of the lane id: computed ahead of the layer loop it cost the
    // loop a register and a scratch slot)
    int l2 = l;
    asm volatile("" : "+v"(l2));
    const int T2 = WR_TILE[16 * g + (l2 & 15)];
    const int ty = T2 / WR_TW, tx = T2 - ty * WR_TW, kk = l2 >> 4;
    const int oc_base = 16 * q + 4 * kk;
    const int gy0 = Y0 + 2 * ty, gx0 = X0 + 2 * tx;
    const bool live = gy0 < a.h && gx0 < a.w;
    const float* src = s_act + (a.nlayer & 1) * (WR_NC * WR_CS);
    const int cb = kk * WR_CS + (2 * ty + 1) * WR_RS + (2 * tx + 1);
    f32x4 ca[WT_NP];
#pragma unroll
    for (int p = 0; p < WT_NP; ++p) ca[p] = f32x4{0.f, 0.f, 0.f, 0.f};
    const f32x4* cu = reinterpret_cast<const f32x4*>(a.ct_u) + (size_t)(q * 3) * 64 + l2;
    constexpr size_t CSTEP = (size_t)4 * 3 * 64;
    constexpr int CT_NKS = WR_NC / 4;
    // (weights: the same hand-written request / wait pairs as the layers' -- see load_u; three 16-byte loads per block)
#if WR_UASM
    auto load_w = [&](int ks, f32x4 (&w)[3]) {
      const f32x4* pw = cu + (size_t)(ks < CT_NKS ? ks : CT_NKS - 1) * CSTEP;
      asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(w[0]) : "v"(pw));
      asm volatile("global_load_dwordx4 %0, %1, off offset:1024" : "=v"(w[1]) : "v"(pw));
      asm volatile("global_load_dwordx4 %0, %1, off offset:2048" : "=v"(w[2]) : "v"(pw));
    };
    auto wait_w = [&](f32x4 (&w)[3]) {
      asm volatile("s_waitcnt vmcnt(5)" : "+v"(w[0]));
      asm volatile("s_waitcnt vmcnt(4)" : "+v"(w[1]));
      asm volatile("s_waitcnt vmcnt(3)" : "+v"(w[2]));
    };
    // (the last two requests are never used: keep their registers until they have landed -- see drain_u)
    auto drain_w = [&](f32x4 (&wa)[3], f32x4 (&wb_)[3]) {
      asm volatile("s_waitcnt vmcnt(0)" : "+v"(wa[0]), "+v"(wa[1]), "+v"(wa[2]), "+v"(wb_[0]), "+v"(wb_[1]), "+v"(wb_[2]));
    };
#else
    auto load_w = [&](int ks, f32x4 (&w)[3]) {
      if (ks >= CT_NKS) return;
      const f32x4* pw = cu + (size_t)ks * CSTEP;
      w[0] = pw[0]; w[1] = pw[64]; w[2] = pw[128];
    };
    auto wait_w = [&](f32x4 (&)[3]) {};
    auto drain_w = [&](f32x4 (&)[3], f32x4 (&)[3]) {};
#endif
    // one K step: window, weight sums, input transform -> 25 MFMAs in the order of the products (see above)
    auto cstep = [&](int ks, f32x4 (&w)[3]) {
      wait_w(w);
      const float* sp = src + cb + ks * (4 * WR_CS);
      float d[3][3];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) d[i][j] = sp[i * WR_RS + j];
      auto W = [&](int ky, int kx) { return w[(ky * 3 + kx) >> 2][(ky * 3 + kx) & 3]; };
      auto mm = [&](int p, float wv, float bv) { ca[p] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv, bv, ca[p], 0, 0, 0); };
      // phase (0,0)
#pragma unroll
      for (int ya = 0; ya < 2; ++ya)
#pragma unroll
        for (int xb = 0; xb < 2; ++xb) mm(2 * ya + xb, W(1, 1), d[ya][xb]);
      // phase (0,1): x-transform of each window row (the third row is needed by phase (1,1) only)
      float c3[3][3];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        c3[i][0] = d[i][0] - d[i][1];
        c3[i][1] = d[i][1];
        c3[i][2] = d[i][2] - d[i][1];
      }
      {
        const float gx[3] = {W(1, 2), W(1, 2) + W(1, 0), W(1, 0)};
#pragma unroll
        for (int ya = 0; ya < 2; ++ya)
#pragma unroll
          for (int j = 0; j < 3; ++j) mm(4 + 3 * ya + j, gx[j], c3[ya][j]);
      }
      // phase (1,0): y-transform of the two columns
      {
        const float gy[3] = {W(2, 1), W(2, 1) + W(0, 1), W(0, 1)};
#pragma unroll
        for (int xb = 0; xb < 2; ++xb) {
          mm(10 + xb, gy[0], d[0][xb] - d[1][xb]);
          mm(12 + xb, gy[1], d[1][xb]);
          mm(14 + xb, gy[2], d[2][xb] - d[1][xb]);
        }
      }
      // phase (1,1): both transforms; G's middle row is the row sum of the column sums
      {
        const float g0[3] = {W(2, 2), W(2, 2) + W(2, 0), W(2, 0)};
        const float g2[3] = {W(0, 2), W(0, 2) + W(0, 0), W(0, 0)};
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          mm(16 + j, g0[j], c3[0][j] - c3[1][j]);
          mm(19 + j, g0[j] + g2[j], c3[1][j]);
          mm(22 + j, g2[j], c3[2][j] - c3[1][j]);
        }
      }
    };
    f32x4 w0[3], w1[3];
    load_w(0, w0);
    load_w(1, w1);
    for (int ks = 0; ks < CT_NKS; ks += 2) {
      cstep(ks, w0);
      __builtin_amdgcn_sched_barrier(0);
      load_w(ks + 2, w0);
      __builtin_amdgcn_sched_barrier(0);
      cstep(ks + 1, w1);
      __builtin_amdgcn_sched_barrier(0);
      load_w(ks + 3, w1);
      __builtin_amdgcn_sched_barrier(0);
    }
    drain_w(w0, w1);
    if (live) {
      const float cslope = act_slope(a.ct_act);
      const size_t ohw = (size_t)4 * hw;
      const int ow = 2 * a.w;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float bz = a.ct_bias[oc_base + r];
        float* yo = a.ct_y + (size_t)(oc_base + r) * ohw + (size_t)(2 * gy0) * ow + 2 * gx0;
#pragma unroll
        for (int ya = 0; ya < 2; ++ya) {      // input row ya of the tile: HR rows 2 ya, 2 ya + 1
          float o[2][4];                      // [py][column 2 xb + px]
          float s3[3];
#pragma unroll
          for (int j = 0; j < 3; ++j) s3[j] = ca[16 + 3 * ya + j][r] + ca[16 + 3 * (ya + 1) + j][r];
#pragma unroll
          for (int xb = 0; xb < 2; ++xb) {
            o[0][2 * xb] = ca[2 * ya + xb][r];
            o[0][2 * xb + 1] = ca[4 + 3 * ya + xb][r] + ca[4 + 3 * ya + xb + 1][r];
            o[1][2 * xb] = ca[10 + 2 * ya + xb][r] + ca[10 + 2 * (ya + 1) + xb][r];
            o[1][2 * xb + 1] = s3[xb] + s3[xb + 1];
          }
#pragma unroll
          for (int py = 0; py < 2; ++py) {
            float o4[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float v = o[py][e] + bz;
              o4[e] = __builtin_fmaxf(v, cslope * v);
            }
            *reinterpret_cast<float4*>(yo + (size_t)(2 * ya + py) * ow) = make_float4(o4[0], o4[1], o4[2], o4[3]);
          }
        }
      }
    }
  }
}

// SRNet's first ConvTranspose2d weights (cin 64, cout 64, 3, 3) -> the tail's A operands:
// [K step 16][channel block 4][j 3][lane 64][e 4]: element p = 4 j + e < 9 of lane (oc = 16 q + (lane & 15),
// ic = 4 ks + (lane >> 4)) is W[ic][oc][p / 3][p % 3]; p >= 9 is padding.
__global__ void wres_ct_pack_kernel(const float* __restrict__ w, float* __restrict__ out) {
  const int total = 16 * 4 * 3 * 64 * 4;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int e = i & 3, lane = (i >> 2) & 63;
    int t = i >> 8;
    const int j = t % 3; t /= 3;
    const int qq = t & 3, ks = t >> 2;
    const int p = 4 * j + e;
    const int oc = 16 * qq + (lane & 15), ic = 4 * ks + (lane >> 4);
    out[i] = p < 9 ? w[((size_t)ic * WR_NC + oc) * 9 + p] : 0.f;
  }
}

static long long wres_blocks(int h, int w) { return (long long)cdiv(h, WR_BH) * cdiv(w, WR_BW); }

// one workgroup per CU, and a few CUs left free so that a co-running launch (the flow estimator on
// its own stream) cannot keep the last workgroups of this one from ever starting
bool conv3x3_wino_resident_ok(int n, int cout, int h, int w) {
  if (n != 1 || cout != WR_NC || h < 2 || w < 2 || (h & 1) || (w & 1)) return false;
  const int cap = resident_capacity<conv3x3_wino_resident_kernel>(WR_THREADS, WR_LDS_BYTES);
  return cap > 0 && wres_blocks(h, w) <= cap - 8 && wres_blocks(h, w) <= 1023;   // (1023: the ring table's 16-bit owner field)
}

int64_t conv3x3_wino_resident_ws_bytes(int h, int w) {
  const long long nb = wres_blocks(h, w);
  return 2 * nb * WR_SLOTS * WR_NC * 8 + 256;   // exchange granules ({value, tag} pairs) + fault counter
}

int conv3x3_wino_resident_launch(const tg_wino_layer* layers, int n_layers, int cout, int h, int w, void* ws,
                                 int32_t* err, unsigned base, int poll_limit, tg_stream_t stream,
                                 const tg_wres_convt* ct) {
  TG_REQUIRE(layers && ws && err, TG_E_ARG, "conv3x3_wino_resident: null pointer");
  TG_REQUIRE(n_layers >= 1 && n_layers <= WR_MAXL, TG_E_ARG, "conv3x3_wino_resident: %d layers (1..%d)", n_layers, WR_MAXL);
  TG_REQUIRE(conv3x3_wino_resident_ok(1, cout, h, w), TG_E_SHAPE,
             "conv3x3_wino_resident: cout=%d h=%d w=%d not supported (cout 64, even h and w, one 8x24 block per CU)", cout, h, w);
  TG_REQUIRE(((uintptr_t)ws % 256) == 0, TG_E_ARG, "conv3x3_wino_resident: workspace must be 256-byte aligned");
  WResArgs a{};
  a.nlayer = n_layers; a.h = h; a.w = w; a.nbx = cdiv(w, WR_BW); a.nby = cdiv(h, WR_BH);
  const long long nb = (long long)a.nbx * a.nby;
  for (int i = 0; i < n_layers; ++i) {
    const tg_wino_layer& l = layers[i];
    TG_REQUIRE(l.x && l.u_packed && l.y && l.bias, TG_E_ARG, "conv3x3_wino_resident: layer %d: null pointer", i);
    TG_REQUIRE(l.act == TG_ACT_NONE || l.act == TG_ACT_RELU || l.act == TG_ACT_LRELU02, TG_E_ARG,
               "conv3x3_wino_resident: layer %d: act=%d", i, l.act);
    if (i == 0) {
      TG_REQUIRE(l.cin > 0 && l.cin <= WR_NC && (!l.x2 || (l.c1 > 0 && l.c1 < l.cin)) && !l.res, TG_E_ARG,
                 "conv3x3_wino_resident: first layer: cin=%d (<= 64) c1=%d, no residual", l.cin, l.c1);
    } else {
      // the chain pattern of the reference's SRNet: a layer reads what the previous one wrote; a residual
      // input is the tensor the previous layer read (= what the destination LDS buffer still holds)
      TG_REQUIRE(l.cin == cout && !l.x2 && l.x == layers[i - 1].y, TG_E_ARG,
                 "conv3x3_wino_resident: layer %d must read layer %d's output", i, i - 1);
      TG_REQUIRE(!l.res || l.res == layers[i - 1].x, TG_E_ARG,
                 "conv3x3_wino_resident: layer %d: the residual input must be layer %d's input", i, i - 1);
    }
    WResLayer& d = a.L[i];
    // (K steps: whole pairs up to cin, not whole 16-channel stages of U -- a step over channels that do not exist adds
    // exact zeros (both LDS buffers are zero-filled); U is packed in whole stages, so the block index stays in range)
    d.u = l.u_packed; d.bias = l.bias; d.act = l.act; d.res = l.res ? 1 : 0; d.nks = 2 * cdiv(l.cin, 8);
  }
  a.x = layers[0].x; a.x2 = layers[0].x2; a.c1 = layers[0].x2 ? layers[0].c1 : layers[0].cin; a.cin0 = layers[0].cin;
  a.y = layers[n_layers - 1].y;
  // (the last layer's 2 x 2 tiles leave as float2 rows at even offsets of an even map; one rule with and without the tail)
  TG_REQUIRE(((uintptr_t)a.y % 8) == 0, TG_E_ARG, "conv3x3_wino_resident: the last layer's y must be 8-byte aligned");
  a.xbuf = static_cast<float*>(ws);
  a.err = err; a.base = base; a.poll_limit = poll_limit;
  if (ct) {
    TG_REQUIRE(ct->u_packed && ct->bias && ct->y, TG_E_ARG, "conv3x3_wino_resident: transposed-conv tail: null pointer");
    TG_REQUIRE(ct->act == TG_ACT_NONE || ct->act == TG_ACT_RELU || ct->act == TG_ACT_LRELU02, TG_E_ARG,
               "conv3x3_wino_resident: transposed-conv tail: act=%d", ct->act);
    TG_REQUIRE(n_layers + 1 < 32 && ((uintptr_t)ct->y % 16) == 0, TG_E_ARG, "conv3x3_wino_resident: transposed-conv tail: layers / alignment");
    a.ct_u = ct->u_packed; a.ct_bias = ct->bias; a.ct_y = ct->y; a.ct_act = ct->act;
  }
  hipLaunchKernelGGL(conv3x3_wino_resident_kernel, dim3((unsigned)nb), dim3(WR_THREADS), WR_LDS_BYTES,
                     (hipStream_t)stream, a);
  return check_launch("conv3x3_wino_resident");
}

}  // namespace tg

using namespace tg;

extern "C" int tg_conv3x3_wino_resident_supported(int n, int cout, int h, int w) {
  return conv3x3_wino_resident_ok(n, cout, h, w) ? 1 : 0;
}

extern "C" int64_t tg_conv3x3_wino_resident_ws_bytes(int h, int w) {
  if (h <= 0 || w <= 0) return -1;
  return conv3x3_wino_resident_ws_bytes(h, w);
}

extern "C" int tg_conv3x3_wino_resident_ring_item(int h, int w, int block, int ring_pixel, int* owner_block,
                                                  int* owner_slot, int* lds_offset) {
  TG_REQUIRE(owner_block && owner_slot && lds_offset, TG_E_ARG, "conv3x3_wino_resident_ring_item: null pointer");
  TG_REQUIRE(h >= 2 && w >= 2 && !(h & 1) && !(w & 1), TG_E_SHAPE, "conv3x3_wino_resident_ring_item: h=%d w=%d (even, >= 2)", h, w);
  const int nbx = cdiv(w, WR_BW);
  TG_REQUIRE(block >= 0 && block < wres_blocks(h, w) && ring_pixel >= 0 && ring_pixel < WR_NRING, TG_E_ARG,
             "conv3x3_wino_resident_ring_item: block %d of %lld, ring pixel %d of %d", block, wres_blocks(h, w), ring_pixel, WR_NRING);
  const WResRingItem it = wres_ring_item(h, w, nbx, block % nbx, block / nbx, ring_pixel);
  *owner_block = it.owner; *owner_slot = it.slot; *lds_offset = it.lds;
  return it.valid;
}

extern "C" int tg_conv3x3_wino_resident(const tg_wino_layer* layers, int n_layers, int cout, int h, int w,
                                        void* workspace, int epoch, tg_stream_t stream) {
  return tg_conv3x3_wino_resident_ct(layers, n_layers, cout, h, w, workspace, epoch, nullptr, stream);
}

extern "C" int tg_conv3x3_wino_resident_ct(const tg_wino_layer* layers, int n_layers, int cout, int h, int w,
                                           void* workspace, int epoch, const tg_wres_convt* convt, tg_stream_t stream) {
  TG_REQUIRE(workspace && epoch > 0, TG_E_ARG, "conv3x3_wino_resident: bad argument (epoch counts from 1)");
  const int64_t bytes = conv3x3_wino_resident_ws_bytes(h, w);
  int32_t* err = reinterpret_cast<int32_t*>(static_cast<char*>(workspace) + bytes - 256);
  return conv3x3_wino_resident_launch(layers, n_layers, cout, h, w, workspace, err, (unsigned)epoch * 32u,
                                      TG_CHAIN_POLL_LIMIT_DEFAULT, stream, convt);
}

extern "C" size_t tg_conv3x3_wino_resident_ct_floats(void) { return (size_t)16 * 4 * 3 * 64 * 4; }

extern "C" int tg_conv3x3_wino_resident_ct_pack(const float* w_iohw, float* out, tg_stream_t stream) {
  TG_REQUIRE(w_iohw && out, TG_E_ARG, "conv3x3_wino_resident_ct_pack: null pointer");
  hipLaunchKernelGGL(wres_ct_pack_kernel, dim3(96), dim3(256), 0, (hipStream_t)stream, w_iohw, out);
  return check_launch("conv3x3_wino_resident_ct_pack");
}
