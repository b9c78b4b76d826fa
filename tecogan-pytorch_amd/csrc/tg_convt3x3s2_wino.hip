// Z mode of ConvTranspose2d(64, 64, 3, 2, 1, 1) in the Winograd domain (inference's last up-sampling layer; the
// output conv's channel contraction in the epilogue, as convt3x3s2_mfma_kernel<., ., true>).
//
// Along x, the px = 1 outputs of an input column pair (x, x + 1) are a 2-tap correlation (tap conventions of
// tg_convt3x3s2_mfma.hip: px = 0 uses kx = 1 at x; px = 1 uses kx = 2 at x and kx = 0 at x + 1), so F(2,2) applies
// with coefficients +-1:
//   d0 = in[x] - in[x+1]   d1 = in[x+1]            d2 = in[x+2] - in[x+1]
//   g0 = W[kx2]            g1 = W[kx2] + W[kx0]    g2 = W[kx0]
//   y(x) = g0 d0 + g1 d1   y(x+1) = g1 d1 + g2 d2
// Rows likewise.  Per 2x2 tile of input pixels (16 HR outputs, 3x3 input window) the four phases need
// 4 + 6 + 6 + 9 = 25 products instead of 36 (phase (0,0) raw, (0,1) F(2,2) in x, (1,0) in y, (1,1) F(2x2,2x2)),
// against 16 distinct weight matrices (9 raw taps, 7 sums: tg_convt_pack_wino).
//
// Workgroup = 4 waves = one 2-row x 32-column input strip (16 tiles) x 64 output channels; wave q holds output
// channels [16 q, 16 q + 16) x the 16 tiles as 25 accumulators of v_mfma_f32_16x16x4_f32 (100 registers):
// register r of lane l is channel 16 q + 4 (l >> 4) + r of tile l & 15.
//   * input: 16-channel chunks, double-buffered in LDS AFTER the input transform (the 25 B values per channel and
//     tile are computed once per chunk by the whole workgroup -- thread (wave s, lane l) transforms channel
//     4 (l >> 4) + s of tile l & 15 -- not once per wave); a product's B operand is one ds_read_b128 per lane
//     (4 k-steps: channels 4 (l >> 4) + s, s = 0..3);
//   * weights: each wave's 16 x 16 x 16 slice of the 16 matrices per chunk goes L2 -> registers (a matrix of the next
//     chunk is requested right after its last use in this one: 64 registers, one chunk of latency hiding);
//   * epilogue: output transform (additions of accumulators with the same lane mapping; the bias was the initial value
//     of one accumulator per output), activation, then
//     the output conv's contraction with the accumulator layout as the B operand of 16x16x4 MFMAs (B[k][col] =
//     register r of lane (k, col) = channel 16 q + 4 k + r), one input row of the tile at a time; the four waves'
//     partial tap planes meet in LDS and are summed in the fixed order q0 + q1 + q2 + q3, each wave storing a
//     quarter as 16-byte rows of four HR pixels.
// Every output's arithmetic depends only on its strip, never on the grid, n or how the launch is split.
// (Built with -fno-slp-vectorize, the configuration measured in EXPERIMENTS.md.)
// TG_FILE_FLAGS: -fno-slp-vectorize
#include "tg_common.h"
#include "tg_launch.h"

namespace tg {

constexpr int WZ_TILES = 16;                                   // 2x2 tiles per strip
constexpr int WZ_NP = 25;                                      // products per tile and channel
constexpr int WZ_NA = 16;                                      // transformed weight matrices
constexpr int WZ_CH = 16;                                      // input channels per staged chunk
constexpr int WZ_NCH = 4;                                      // chunks (cin <= 64)
constexpr int WZ_B_FLOATS = WZ_NP * WZ_CH * WZ_TILES;          // [p 25][k 4][tile 16][s 4]
constexpr int WZ_RED_FLOATS = 4 * 2 * 32 * WZ_TILES * 4;       // [wave 4][HR row 2][m 32][tile 16][HR col 4]
constexpr size_t WZ_LDS_BYTES = (size_t)(WZ_RED_FLOATS > 2 * WZ_B_FLOATS ? WZ_RED_FLOATS : 2 * WZ_B_FLOATS) * sizeof(float);

struct ConvTWinoArgs {
  const float* x;
  const float* wa;        // tg_convt_pack_wino: [chunk 4][matrix 16][k 4][oc 64][s 4], channel 16 chunk + 4 k + s
  const float* bias;
  const float* wz;        // tg_convt_pack_wz (the direct Z form's contraction operand, read in this kernel's order)
  float* z;               // (n, 32, 2h, 2w) planes; the first zrows are written
  long long x_ns, z_ns;
  int cin, cout, h, w, act, zrows;
  int tiles_x;            // 32-column strips per row
  int strips_y;           // strip rows of this launch
  int strip_base;         // first strip row of this launch (0 but for the second launch of a split)
};

// product p -> (weight matrix, B value); the B values of a tile are ordered as the products
//  p  0.. 3  phase (0,0): raw in[a][b]                         matrix 0 = W[1][1]
//  p  4.. 9  phase (0,1): row a, x-transform j: p = 4 + 3a + j    matrix 1 + j
//  p 10..15  phase (1,0): y-transform i, column b: p = 10 + 2i + b   matrix 4 + i
//  p 16..24  phase (1,1): y-transform i, x-transform j: p = 16 + 3i + j   matrix 7 + 3i + j
__host__ __device__ constexpr int wz_matrix(int p) {
  return p < 4 ? 0 : (p < 10 ? 1 + (p - 4) % 3 : (p < 16 ? 4 + (p - 10) / 2 : 7 + (p - 16)));
}
// issue order of the products: grouped by matrix (0 1 2 3 | 4 7 | 5 8 | 6 9 | 10 11 | ... | 24), taken in pairs
__host__ __device__ constexpr int wz_order(int i) { return (i < 4 || i >= 10) ? i : 4 + ((i - 4) >> 1) + 3 * ((i - 4) & 1); }
constexpr int WZ_PAIRS = (WZ_NP + 1) / 2;
// the pair of wz_order() that holds matrix m's last product
__host__ __device__ constexpr int wz_last_pair(int m) { return m == 0 ? 1 : (m <= 6 ? m + 1 : (m + 9) >> 1); }

// RELU: the activation is ReLU (else x >= 0 ? x : slope x); TWO: tap-plane rows 16.. exist (cz >= 2) -- compile-time, so
// the epilogue has no per-element branch
template <bool RELU, bool TWO>
__global__ __launch_bounds__(256, 2) void convt3x3s2_wino_z_kernel(ConvTWinoArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int b = blockIdx.x;
  const int tx = b % a.tiles_x; b /= a.tiles_x;
  const int sy = b % a.strips_y;
  const int n = b / a.strips_y;
  const int x0 = tx * 32, y0 = 2 * (a.strip_base + sy);
  const int hw = a.h * a.w;
  const unsigned plane = (unsigned)hw * 4u;
  const int lk = lane >> 4, lt = lane & 15;

  // ---- staging role: channel 4 lk + wave of each chunk, tile lt: the 3x3 window rows y0 .. y0 + 2, columns
  // x0 + 2 lt .. + 2 (outside the image: 0 -- a column past the row's end would read the next row, hence the offsets)
  const __amdgpu_buffer_rsrc_t rx = TG_BUF_RSRC(a.x + (long long)n * a.x_ns, a.cin * hw * 4);
  // (offsets of chunk 0; the chunk's channel offset is added to the VECTOR offset, so that a channel past cin is out of
  // the descriptor's range whatever the scalar offset: a zero)
  unsigned co[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int gy = y0 + i, gx = x0 + 2 * lt + j;
      co[i][j] = (gy < a.h && gx < a.w) ? (unsigned)(4 * lk + wave) * plane + (unsigned)(gy * a.w + gx) * 4u : BUF_OOB;
    }
  float raw[3][3];
  auto load_raw = [&](int c) {
    const unsigned cb = (unsigned)(c * WZ_CH) * plane;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j)
        raw[i][j] = buf_ld<float>(rx, co[i][j] + cb);
  };
  // the 16 subtractions of the input transform and the 25 B values into LDS buffer buf
  auto store_b = [&](int buf) {
    float c3[3][3];                                            // x-transform of each window row
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      c3[i][0] = raw[i][0] - raw[i][1];
      c3[i][1] = raw[i][1];
      c3[i][2] = raw[i][2] - raw[i][1];
    }
    float v[WZ_NP];
#pragma unroll
    for (int ya = 0; ya < 2; ++ya)
#pragma unroll
      for (int xb = 0; xb < 2; ++xb) v[2 * ya + xb] = raw[ya][xb];
#pragma unroll
    for (int ya = 0; ya < 2; ++ya)
#pragma unroll
      for (int j = 0; j < 3; ++j) v[4 + 3 * ya + j] = c3[ya][j];
#pragma unroll
    for (int xb = 0; xb < 2; ++xb) {
      v[10 + xb] = raw[0][xb] - raw[1][xb];
      v[12 + xb] = raw[1][xb];
      v[14 + xb] = raw[2][xb] - raw[1][xb];
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      v[16 + j] = c3[0][j] - c3[1][j];
      v[19 + j] = c3[1][j];
      v[22 + j] = c3[2][j] - c3[1][j];
    }
    float* sb = smem + buf * WZ_B_FLOATS + lane * 4 + wave;
#pragma unroll
    for (int p = 0; p < WZ_NP; ++p) sb[p * 256] = v[p];
  };

  // ---- this wave's weights: lane (lk, lt) holds matrix m's channels 4 lk + s (s = 0..3) of output channel 16 wave + lt
  // (a buffer resource: the lane's part once, the (chunk, matrix) block as the scalar offset -- no 64-bit addresses)
  const __amdgpu_buffer_rsrc_t rwa = TG_BUF_RSRC(a.wa, TG_CONVT_WINO_FLOATS * 4);
  const unsigned wvo = (unsigned)(lk * 64 + 16 * wave + lt) * 16u;
  auto lda = [&](int c, int m) {
    return buf_ld<f32x4>(rwa, wvo, (c * WZ_NA + m) * 4096);
  };
  f32x4 A[WZ_NA];
  // The bias rides in the accumulators: every output of the output transform sums exactly one of the products
  // 0..3, 5, 8, 12, 13, 20 (phase (0,0) itself; the middle term of the F(2,2) sums; M11[1][1] in all four of (1,1)).
  f32x4 acc[WZ_NP];
  {
    float bs[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int oc = 16 * wave + 4 * lk + r;
      bs[r] = (a.bias && oc < a.cout) ? a.bias[oc] : 0.f;
    }
#pragma unroll
    for (int p = 0; p < WZ_NP; ++p) {
      const bool with_bias = p < 4 || p == 5 || p == 8 || p == 12 || p == 13 || p == 20;
      acc[p] = with_bias ? f32x4{bs[0], bs[1], bs[2], bs[3]} : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }

#pragma unroll
  for (int m = 0; m < WZ_NA; ++m) A[m] = lda(0, m);
  load_raw(0);
  store_b(0);
  __syncthreads();

  // The K loop: four chunks (channels past cin are zeros of the input and of the pack), straight-line code -- no
  // branch, so the waits are exact: a chunk's B values are read from LDS one pair of products ahead, the two products of
  // a pair are interleaved (a 16x16x4 MFMA's dependent latency is 40 cycles against 32 of issue), and a matrix of the
  // next chunk is requested after the pair that holds its last use in this one.
#pragma unroll
  for (int c = 0; c < WZ_NCH; ++c) {
    const bool more = c + 1 < WZ_NCH;                          // compile-time
    if (more) load_raw(c + 1);
    const float* sb = smem + (c & 1) * WZ_B_FLOATS + lane * 4;
    f32x4 bq[2][2];
    bq[0][0] = *reinterpret_cast<const f32x4*>(sb + wz_order(0) * 256);
    bq[0][1] = *reinterpret_cast<const f32x4*>(sb + wz_order(1) * 256);
#pragma unroll
    for (int g = 0; g < WZ_PAIRS; ++g) {
      const int p0 = wz_order(2 * g), p1 = 2 * g + 1 < WZ_NP ? wz_order(2 * g + 1) : -1;
      if (g + 1 < WZ_PAIRS) {
        bq[(g + 1) & 1][0] = *reinterpret_cast<const f32x4*>(sb + wz_order(2 * g + 2) * 256);
        if (2 * g + 3 < WZ_NP) bq[(g + 1) & 1][1] = *reinterpret_cast<const f32x4*>(sb + wz_order(2 * g + 3) * 256);
      }
#pragma unroll
      for (int s = 0; s < 4; ++s) {                         // (in this order: left alone, the scheduler chains them)
        acc[p0] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[wz_matrix(p0)][s], bq[g & 1][0][s], acc[p0], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        if (p1 >= 0) acc[p1] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[wz_matrix(p1)][s], bq[g & 1][1][s], acc[p1], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
      if (more) {
#pragma unroll
        for (int m = 0; m < WZ_NA; ++m)
          if (wz_last_pair(m) == g) A[m] = lda(c + 1, m);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    if (more) store_b((c + 1) & 1);
    __syncthreads();
  }

  // ---- epilogue: output transform, activation, contraction with conv_out's weights, planes ----
  const float slope = act_slope(a.act);
  // contraction operand: A[m][k] = Wout[m][16 wave + 4 k + r] for m = 16 h + lt, read from the direct form's pack
  // (wz[(half * 16 + r') * 64 + l'] holds (m = l' & 31, c = 32 half + (r' & 3) + 8 (r' >> 2) + 4 (l' >> 5)))
  float az[2][4];
#pragma unroll
  for (int hh = 0; hh < 2; ++hh)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = 16 * wave + 4 * lk + r, cc = c & 31;
      const int m = 16 * hh + lt;
      az[hh][r] = a.wz[((c >> 5) * 16 + (cc & 3) + 4 * (cc >> 3)) * 64 + ((cc >> 2) & 1) * 32 + m];
    }
  constexpr bool two_halves = TWO;
  auto actv = [&](float t) { return RELU ? fmaxf(t, 0.f) : (t >= 0.f ? t : t * slope + 0.f); };
  const int ow = 2 * a.w;
  const unsigned ohw = 4u * (unsigned)hw;
  const __amdgpu_buffer_rsrc_t rz = TG_BUF_RSRC(a.z + (long long)n * a.z_ns, (int)(32u * ohw * 4u));
  float* const red_w = smem + (wave * 2 * 32 + 4 * lk) * WZ_TILES * 4 + lt * 4;   // + ((R2 * 32 + 16 h + r) * 16) * 4
#pragma unroll
  for (int ya = 0; ya < 2; ++ya) {                             // input row y0 + ya of the tile: HR rows 2 ya, 2 ya + 1
    // HR values o[R2][C] (R2 = py, C = 2 xb + px) of this row, channel register r
    f32x4 zp[2][4][2];                                         // [R2][C][m half]
#pragma unroll
    for (int R2 = 0; R2 < 2; ++R2)
#pragma unroll
      for (int C = 0; C < 4; ++C)
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) zp[R2][C][hh] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float o[2][4];
      // (py 0, px 0): raw; (py 0, px 1): F(2,2) in x; (py 1, px 0): in y; (py 1, px 1): both, rows summed first
#pragma unroll
      for (int xb = 0; xb < 2; ++xb) {
        o[0][2 * xb] = acc[2 * ya + xb][r];
        o[0][2 * xb + 1] = acc[4 + 3 * ya + xb][r] + acc[4 + 3 * ya + xb + 1][r];
        o[1][2 * xb] = acc[10 + 2 * ya + xb][r] + acc[10 + 2 * (ya + 1) + xb][r];
      }
      float s3[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) s3[j] = acc[16 + 3 * ya + j][r] + acc[16 + 3 * (ya + 1) + j][r];
#pragma unroll
      for (int xb = 0; xb < 2; ++xb) o[1][2 * xb + 1] = s3[xb] + s3[xb + 1];
#pragma unroll
      for (int R2 = 0; R2 < 2; ++R2)
#pragma unroll
        for (int C = 0; C < 4; ++C) {
          const float v = actv(o[R2][C]);
          zp[R2][C][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(az[0][r], v, zp[R2][C][0], 0, 0, 0);
          if constexpr (two_halves) zp[R2][C][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(az[1][r], v, zp[R2][C][1], 0, 0, 0);
        }
    }
    // partial planes of this wave: lane (lk, lt) holds m = 16 h + 4 lk + e of tile lt at HR (R2, C)
#pragma unroll
    for (int R2 = 0; R2 < 2; ++R2)
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        if (hh == 1 && !two_halves) continue;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          *reinterpret_cast<f32x4*>(red_w + ((R2 * 32 + 16 * hh + e) * WZ_TILES) * 4) =
              f32x4{zp[R2][0][hh][e], zp[R2][1][hh][e], zp[R2][2][hh][e], zp[R2][3][hh][e]};
      }
    __syncthreads();
    // wave q sums and stores 4 of the 16 (HR row, m block of 4, tile) groups of each lane: fixed order q0 + q1 + q2 + q3
    const int gyin = y0 + ya;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int R2 = i >> 1, hh = i & 1;
      const int m = 16 * hh + 4 * wave + lk;
      if (hh == 1 && !two_halves) continue;
      const float* rr = smem + ((R2 * 32 + m) * WZ_TILES + lt) * 4;
      f32x4 s = *reinterpret_cast<const f32x4*>(rr);
#pragma unroll
      for (int q = 1; q < 4; ++q) s += *reinterpret_cast<const f32x4*>(rr + q * (2 * 32 * WZ_TILES * 4));
      const int xin = x0 + 2 * lt;                             // the tile's first input column: HR columns 2 xin .. + 3
      if (gyin < a.h && m < a.zrows && xin < a.w) {
        const unsigned zo = ((unsigned)m * ohw + (unsigned)((2 * gyin + R2) * ow + 2 * xin)) * 4u;
        if (xin + 1 < a.w) {
          buf_st(s, rz, zo);
        } else {                                               // last column of an odd-width row: two HR pixels
          // (locals first: __builtin_bit_cast of a vector ELEMENT expression reads element 0 whatever the index)
          const float e0 = s[0], e1 = s[1];
          const u32x2 v2 = {__builtin_bit_cast(unsigned, e0), __builtin_bit_cast(unsigned, e1)};
          buf_st(v2, rz, zo);
        }
      }
    }
    if (ya == 0) __syncthreads();                              // the second row re-uses the reduction buffer
  }
}

// W^ from the direct form's packed weights (tg_conv3x3_pack(transposed = 1, ocb = 64): [chunk 8][tap 9][half 2][oc 64][4],
// channel 8 chunk + 4 half + j, value W[ci][oc][tap = ky * 3 + kx]).  Matrix order of wz_matrix(): 0 W11; 1..3 the
// x-transform (g0, g1, g2) = (W12, W12 + W10, W10); 4..6 the y-transform (W21, W21 + W01, W01); 7 + 3 i + j the 2-D
// G[i][j] with rows (W2., W2. + W0., W0.) and columns likewise, the row sum taken of the column sums.
__global__ void convt_pack_wino_kernel(const float* __restrict__ wpk, float* __restrict__ wa, int cin, int cout) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 4 * WZ_NA * 4 * 64 * 4) return;
  const int s = i & 3, oc = (i >> 2) & 63, k = (i >> 8) & 3, mtx = (i >> 10) & 15, c = i >> 14;
  const int ci = 16 * c + 4 * k + s;
  float v = 0.f;
  if (ci < cin && oc < cout) {
    auto W = [&](int ky, int kx) {
      return wpk[((((ci >> 3) * 9 + ky * 3 + kx) * 2 + ((ci >> 2) & 1)) * 64 + oc) * 4 + (ci & 3)];
    };
    // 1-D transforms over the tap index t in {2, sum, 0}: e = 0 -> tap 2, 1 -> tap 2 + tap 0, 2 -> tap 0
    auto gx = [&](int ky, int e) { return e == 0 ? W(ky, 2) : (e == 2 ? W(ky, 0) : W(ky, 2) + W(ky, 0)); };
    if (mtx == 0) v = W(1, 1);
    else if (mtx < 4) v = gx(1, mtx - 1);
    else if (mtx < 7) {
      const int e = mtx - 4;
      v = e == 0 ? W(2, 1) : (e == 2 ? W(0, 1) : W(2, 1) + W(0, 1));
    } else {
      const int ii = (mtx - 7) / 3, jj = (mtx - 7) % 3;
      v = ii == 0 ? gx(2, jj) : (ii == 2 ? gx(0, jj) : gx(2, jj) + gx(0, jj));
    }
  }
  wa[i] = v;
}

// The split of a launch into whole rounds of resident workgroups (2 per CU) and a remainder launch: one image, at least
// one whole round, a remainder (split = 1: whenever a whole round exists; 0: never; -1: the rule = 1).  The rule and the
// launch it governs share this one answer: the strip rows of the first launch, 0 for a single launch.
static int convt_z_wino_split_rows(int n, int h, int w, int split) {
  if (n != 1 || split == 0) return 0;
  const long long tiles_x = cdiv(w, 32), rows = cdiv(h, 2), strips = tiles_x * rows;
  const long long slots = 2ll * device_cus();
  if (strips < slots) return 0;
  const long long rows1 = (strips / slots) * slots / tiles_x;
  return rows1 >= 1 && rows1 < rows ? (int)rows1 : 0;
}

bool convt_z_wino_split_rule(int n, int h, int w, int split) { return convt_z_wino_split_rows(n, h, w, split) > 0; }

template <bool RELU, bool TWO>
static int convt_z_wino_launch(unsigned grid, const ConvTWinoArgs& a, hipStream_t s) {
  if (const int rc = ensure_dynamic_lds<convt3x3s2_wino_z_kernel<RELU, TWO>>(WZ_LDS_BYTES, "convt3x3s2_wino_z")) return rc;
  hipLaunchKernelGGL((convt3x3s2_wino_z_kernel<RELU, TWO>), dim3(grid), dim3(256), WZ_LDS_BYTES, s, a);
  return TG_OK;
}

}  // namespace tg

using namespace tg;

extern "C" int tg_convt_pack_wino(const float* w_packed, float* w_wino, int cin, int cout, tg_stream_t stream) {
  TG_REQUIRE(w_packed && w_wino, TG_E_ARG, "convt_pack_wino: null pointer");
  TG_REQUIRE(cin >= 1 && cin <= 64 && cout >= 1 && cout <= 64, TG_E_SHAPE, "convt_pack_wino: cin=%d cout=%d (<= 64)", cin, cout);
  hipLaunchKernelGGL(convt_pack_wino_kernel, dim3(4 * WZ_NA * 4 * 64 * 4 / 256), dim3(256), 0, (hipStream_t)stream,
                     w_packed, w_wino, cin, cout);
  return check_launch("convt_pack_wino");
}

extern "C" int tg_convt3x3s2_z_wino_fwd(const float* x, int64_t x_nstride, const float* w_wino, const float* bias,
                                        const float* wz, int cz, float* z, int64_t z_nstride, int n, int cin, int cout,
                                        int h, int w, int act, int split, tg_stream_t stream) {
  TG_REQUIRE(x && w_wino && wz && z, TG_E_ARG, "convt3x3s2_z_wino_fwd: null pointer");
  TG_REQUIRE(n > 0 && cin >= 1 && cin <= 64 && cout >= 1 && cout <= 64 && h > 0 && w > 0 && cz >= 1 && 9 * cz <= 32,
             TG_E_SHAPE, "convt3x3s2_z_wino_fwd: n=%d cin=%d (<= 64) cout=%d (<= 64) h=%d w=%d cz=%d (<= 3)", n, cin, cout, h,
             w, cz);
  TG_REQUIRE(act >= TG_ACT_NONE && act <= TG_ACT_LRELU02, TG_E_ARG, "convt3x3s2_z_wino_fwd: act=%d", act);
  TG_REQUIRE(split >= -1 && split <= 1, TG_E_ARG, "convt3x3s2_z_wino_fwd: split=%d (-1 the rule, 0 one launch, 1 split)", split);
  TG_REQUIRE(64ll * h * w * 4 < (1ll << 31) && 32ll * 4 * h * w * 4 < (1ll << 31), TG_E_SHAPE,
             "convt3x3s2_z_wino_fwd: one batch item (input and the 32 planes) must be < 2 GiB");
  // the planes leave as 16-byte (8-byte in the last column of an odd-width map) buffer stores at even float offsets
  // of an image: the same contract as the direct form, so that a caller can swap the two
  TG_REQUIRE((z_nstride % 2) == 0 && ((uintptr_t)z % 8) == 0, TG_E_ARG, "convt3x3s2_z_wino_fwd: z must be 8-byte aligned");
  TG_REQUIRE_NSTRIDE("convt3x3s2_z_wino_fwd", "x", x, x_nstride, n, (long long)cin * h * w);
  TG_REQUIRE_NSTRIDE("convt3x3s2_z_wino_fwd", "z", z, z_nstride, n, 9ll * cz * 4 * h * w);      // the planes it writes
  ConvTWinoArgs a{};
  a.x = x; a.wa = w_wino; a.bias = bias; a.wz = wz; a.z = z; a.x_ns = x_nstride; a.z_ns = z_nstride;
  a.cin = cin; a.cout = cout; a.h = h; a.w = w; a.act = act; a.zrows = 9 * cz;
  a.tiles_x = cdiv(w, 32);
  const int rows = cdiv(h, 2);
  TG_REQUIRE((long long)a.tiles_x * rows * n < (1ll << 31), TG_E_SHAPE, "convt3x3s2_z_wino_fwd: grid");
  hipStream_t s = (hipStream_t)stream;
  const bool relu = act == TG_ACT_RELU, two = cz >= 2;
  auto launch = [&](unsigned grid, const ConvTWinoArgs& args) {
    if (!relu && !two) return convt_z_wino_launch<false, false>(grid, args, s);
    if (!relu) return convt_z_wino_launch<false, true>(grid, args, s);
    if (!two) return convt_z_wino_launch<true, false>(grid, args, s);
    return convt_z_wino_launch<true, true>(grid, args, s);
  };
  if (const int rows1 = convt_z_wino_split_rows(n, h, w, split)) {
    ConvTWinoArgs a1 = a; a1.strips_y = rows1; a1.strip_base = 0;
    if (const int rc = launch((unsigned)(a.tiles_x * rows1), a1)) return rc;
    ConvTWinoArgs a2 = a; a2.strips_y = rows - rows1; a2.strip_base = rows1;
    if (const int rc = launch((unsigned)(a.tiles_x * a2.strips_y), a2)) return rc;
    return check_launch("convt3x3s2_wino_z(split)");
  }
  a.strips_y = rows; a.strip_base = 0;
  if (const int rc = launch((unsigned)(a.tiles_x * rows * n), a)) return rc;
  return check_launch("convt3x3s2_wino_z");
}
