// PNG files of uint8 HWC RGB frames, encoded on the device: what --mode infer writes into a PNG
// folder, without the host's zlib.  The specification is tests/png_ref.py and the bytes must be equal: scanline
// filtering per row, the filtered stream cut into segments of 32768 bytes, every segment deflated on its own with
// Huffman codes only (one dynamic block plus an empty stored block for byte alignment, or one stored block when that
// is not larger), one IDAT.  No LZ77 matches: file size is the price.  tg_png_encode_lz_u8 (further down; DESIGN.md
// section 7n) adds them as a third candidate per segment, behind the same filter, place and finish launches.
//
// Four launches on one stream, ordered by launch order alone -- no workgroup waits for another, no flags, no
// device-wide atomics (the atomics below are all on LDS):
//   png_filter_kernel   workgroup = one row of one frame: the five filter costs, the chosen row into the workspace
//   png_segment_kernel  workgroup = one segment of one frame, held in LDS: histogram, code lengths (rank sort + the
//                       two-queue merge, which pops in the specification's (weight, id) order because merged weights
//                       never decrease and leaf ids are below node ids), canonical codes, bit offsets by a block
//                       prefix sum, codes ORed into LDS words; the segment's bytes, length and Adler sums are staged
//   png_place_kernel    workgroup = one segment: its offset is the sum of the lengths before it; copies the staged
//                       bytes into the file and leaves crc(bytes) * x^(8 * bytes behind them) mod P
//   png_finish_kernel   workgroup = one frame: signature, IHDR, IDAT header, Adler-32 in segment order, the IDAT CRC
//                       (the XOR of the segments' terms: a CRC from a zero register is linear), IEND, the file's size
#include "tg_common.h"
#include "tg_launch.h"

namespace tg {

constexpr int PNG_SEG = 32768;
constexpr int PNG_STAGE = 32784;                // 5 + PNG_SEG, rounded up to 16: one segment's staging region
constexpr int PNG_T = 256;
constexpr int PNG_IN_WORDS = 33 * PNG_T;        // the segment as words; word i lives at i + i / 32 (thread t reads
                                                // words 32 t .. 32 t + 31: a stride of 33 words, no bank shared)
constexpr int PNG_OUT_WORDS = PNG_STAGE / 4;
constexpr int PNG_SEG_LDS = (PNG_IN_WORDS + PNG_OUT_WORDS) * 4;
constexpr int PNG_DYN_HEAD = 3 + 14 + 57 + 1032;   // bits in front of a dynamic block's first code
constexpr int PNG_DATA_AT = 8 + 25 + 8 + 2;     // signature, IHDR, IDAT length and type, 78 01
constexpr unsigned PNG_ADLER = 65521u;
constexpr unsigned CRC_POLY = 0xEDB88320u;

struct png_ws {                                 // the workspace, cut up (all 16-byte aligned)
  uint8_t* filt;                                // n x fpad: the filtered streams
  uint8_t* stage;                               // n x nseg x PNG_STAGE
  unsigned *len, *s1, *s2, *crc;                // n x nseg each
  long long fpad, flen;
  int nseg;
};

static long long png_flen(int h, int w) { return (long long)h * (3LL * w + 1); }
static long long png_nseg(long long flen) { return (flen + PNG_SEG - 1) / PNG_SEG; }
static long long round16(long long v) { return (v + 15) / 16 * 16; }

static long long png_ws_layout(int n, int h, int w, uint8_t* base, png_ws* ws) {
  const long long flen = png_flen(h, w), nseg = png_nseg(flen), fpad = round16(flen), meta = round16(4LL * n * nseg);
  uint8_t* p = reinterpret_cast<uint8_t*>(((uintptr_t)base + 15) & ~(uintptr_t)15);
  long long off = 0;
  ws->filt = p + off;  off += (long long)n * fpad;
  ws->stage = p + off; off += (long long)n * nseg * PNG_STAGE;
  ws->len = reinterpret_cast<unsigned*>(p + off); off += meta;
  ws->s1 = reinterpret_cast<unsigned*>(p + off);  off += meta;
  ws->s2 = reinterpret_cast<unsigned*>(p + off);  off += meta;
  ws->crc = reinterpret_cast<unsigned*>(p + off); off += meta;
  ws->fpad = fpad; ws->flen = flen; ws->nseg = (int)nseg;
  return off + 16;                              // (the alignment of `base` is the caller's business no longer)
}

// ---- filtering -------------------------------------------------------------------------------------------------
__device__ __forceinline__ int png_paeth(int a, int b, int c) {
  const int p = a + b - c;
  const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
__device__ __forceinline__ unsigned png_cost(int v) { v &= 255; return (unsigned)(v >= 128 ? 256 - v : v); }

template <bool ADAPTIVE>
__global__ __launch_bounds__(PNG_T) void png_filter_kernel(const uint8_t* __restrict__ rgb, uint8_t* __restrict__ filt,
                                                           int h, int w, long long fpad) {
  const int r = blockIdx.x, tid = threadIdx.x, row3 = 3 * w;
  const long long k = blockIdx.y;
  const uint8_t* src = rgb + (k * h + r) * (long long)row3;
  const uint8_t* up = src - row3;               // read only when r > 0
  uint8_t* dst = filt + k * fpad + (long long)r * (row3 + 1);
  __shared__ unsigned long long s_cost[5];
  __shared__ int s_type;
  int type = 0;
  if (ADAPTIVE) {
    if (tid < 5) s_cost[tid] = 0;
    __syncthreads();
    unsigned c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0;
    for (int i = tid; i < row3; i += PNG_T) {
      const int x = src[i], a = i >= 3 ? src[i - 3] : 0, b = r > 0 ? up[i] : 0, c = (r > 0 && i >= 3) ? up[i - 3] : 0;
      c0 += png_cost(x);
      c1 += png_cost(x - a);
      c2 += png_cost(x - b);
      c3 += png_cost(x - ((a + b) >> 1));
      c4 += png_cost(x - png_paeth(a, b, c));
    }
    atomicAdd(&s_cost[0], (unsigned long long)c0);
    atomicAdd(&s_cost[1], (unsigned long long)c1);
    atomicAdd(&s_cost[2], (unsigned long long)c2);
    atomicAdd(&s_cost[3], (unsigned long long)c3);
    atomicAdd(&s_cost[4], (unsigned long long)c4);
    __syncthreads();
    if (tid == 0) {
      int best = 0;
      for (int t = 1; t < 5; ++t)
        if (s_cost[t] < s_cost[best]) best = t;   // a tie keeps the lower type
      s_type = best;
    }
    __syncthreads();
    type = s_type;
  }
  if (tid == 0) dst[0] = (uint8_t)type;
  for (int i = tid; i < row3; i += PNG_T) {
    const int x = src[i];
    int pred = 0;
    if (type != 0) {
      const int a = i >= 3 ? src[i - 3] : 0, b = r > 0 ? up[i] : 0, c = (r > 0 && i >= 3) ? up[i - 3] : 0;
      pred = type == 1 ? a : type == 2 ? b : type == 3 ? ((a + b) >> 1) : png_paeth(a, b, c);
    }
    dst[1 + i] = (uint8_t)((x - pred) & 255);
  }
}

// ---- one segment -----------------------------------------------------------------------------------------------
__device__ __forceinline__ void png_put(unsigned* out, unsigned pos, unsigned v, int nbits) {
  const unsigned wd = pos >> 5, sh = pos & 31;
  atomicOr(&out[wd], v << sh);
  if (sh + nbits > 32) atomicOr(&out[wd + 1], v >> (32 - sh));
}

__global__ __launch_bounds__(PNG_T) void png_segment_kernel(const uint8_t* __restrict__ filt, long long fpad,
                                                            long long flen, int nseg, uint8_t* __restrict__ stage,
                                                            unsigned* __restrict__ m_len, unsigned* __restrict__ m_s1,
                                                            unsigned* __restrict__ m_s2) {
  extern __shared__ __attribute__((aligned(16))) unsigned png_smem[];
  unsigned* s_in = png_smem;
  unsigned* s_out = png_smem + PNG_IN_WORDS;
  __shared__ unsigned s_hist[4][260];
  __shared__ unsigned s_cnt[257], s_wt[257], s_sw[257], s_ss[257], s_pl[257], s_len[257], s_code[257];
  __shared__ unsigned s_iw[256], s_pi[256], s_di[256], s_scan[PNG_T], s_blc[16], s_next[16];
  __shared__ unsigned s_n, s_max, s_bits, s_s1;
  __shared__ unsigned long long s_s2;

  const int s = blockIdx.x, tid = threadIdx.x;
  const long long k = blockIdx.y, off = (long long)s * PNG_SEG;
  const int len = (int)(flen - off < PNG_SEG ? flen - off : PNG_SEG);
  const bool last = s == nseg - 1;
  const unsigned* src = reinterpret_cast<const unsigned*>(filt + k * fpad + off);
  const int nw = (len + 3) >> 2;
  for (int wd = tid; wd < PNG_SEG / 4; wd += PNG_T) {
    unsigned v = wd < nw ? src[wd] : 0u;
    if (wd == nw - 1 && (len & 3)) v &= (1u << (8 * (len & 3))) - 1u;     // bytes past the stream are not data
    s_in[wd + (wd >> 5)] = v;
  }
  for (int wd = tid; wd < PNG_OUT_WORDS; wd += PNG_T) s_out[wd] = 0u;
  for (int i = tid; i < 4 * 260; i += PNG_T) (&s_hist[0][0])[i] = 0u;
  if (tid == 0) { s_bits = 0; s_s1 = 0; s_s2 = 0; }
  if (tid < 16) s_blc[tid] = 0;
  __syncthreads();

  // histogram (one per wave) and the Adler sums: S1 = sum of bytes, S2 = sum of (len - index) * byte
  const int b0 = 128 * tid, bn = len - b0 < 128 ? (len - b0 < 0 ? 0 : len - b0) : 128;
  {
    unsigned* hist = s_hist[tid >> 6];
    unsigned s1 = 0, s2 = 0;
    for (int j = 0; j < bn; ++j) {
      const unsigned v = (s_in[33 * tid + (j >> 2)] >> (8 * (j & 3))) & 255u;
      atomicAdd(&hist[v], 1u);
      s1 += v;
      s2 += (unsigned)(len - b0 - j) * v;       // at most 128 * 32768 * 255 < 2^32
    }
    if (bn) {
      atomicAdd(&s_s1, s1);
      atomicAdd(&s_s2, (unsigned long long)s2);
    }
  }
  __syncthreads();
  for (int sym = tid; sym < 257; sym += PNG_T) {
    const unsigned c = sym < 256 ? s_hist[0][sym] + s_hist[1][sym] + s_hist[2][sym] + s_hist[3][sym] : 1u;
    s_cnt[sym] = c;
    s_wt[sym] = c;
  }

  // code lengths; weights are halved (rounding up) and the tree rebuilt while a length exceeds 15
  for (;;) {
    if (tid == 0) { s_n = 0; s_max = 0; }
    __syncthreads();
    for (int sym = tid; sym < 257; sym += PNG_T) {
      const unsigned wt = s_wt[sym];
      s_len[sym] = 0;
      if (wt) {
        unsigned rank = 0;
        for (int q = 0; q < 257; ++q) {
          const unsigned wq = s_wt[q];
          rank += (wq != 0 && (wq < wt || (wq == wt && q < sym))) ? 1u : 0u;
        }
        s_sw[rank] = wt;
        s_ss[rank] = (unsigned)sym;
        atomicAdd(&s_n, 1u);
      }
    }
    __syncthreads();
    const int n = (int)s_n;                     // >= 2: symbol 256 and at least one byte
    if (tid == 0) {
      int li = 0, ii = 0, ni = 0;
      for (int step = 0; step < n - 1; ++step) {
        unsigned wsum = 0;
        for (int q = 0; q < 2; ++q) {
          if (li < n && (ii >= ni || s_sw[li] <= s_iw[ii])) {   // equal weights: the leaf, its id is the lower
            wsum += s_sw[li];
            s_pl[li++] = (unsigned)step;
          } else {
            wsum += s_iw[ii];
            s_pi[ii++] = (unsigned)step;
          }
        }
        s_iw[ni++] = wsum;
      }
      s_di[n - 2] = 0;
      for (int i = n - 3; i >= 0; --i) s_di[i] = s_di[s_pi[i]] + 1;
    }
    __syncthreads();
    for (int i = tid; i < n; i += PNG_T) {
      const unsigned l = s_di[s_pl[i]] + 1;
      s_len[s_ss[i]] = l;
      atomicMax(&s_max, l);
    }
    __syncthreads();
    const unsigned mx = s_max;
    __syncthreads();
    if (mx <= 15) break;
    for (int sym = tid; sym < 257; sym += PNG_T) {
      const unsigned wt = s_wt[sym];
      s_wt[sym] = wt ? (wt + 1) >> 1 : 0;
    }
  }

  for (int sym = tid; sym < 257; sym += PNG_T) {
    const unsigned l = s_len[sym];
    if (l) {
      atomicAdd(&s_bits, s_cnt[sym] * l);
      atomicAdd(&s_blc[l], 1u);
    }
  }
  __syncthreads();
  const unsigned bits = s_bits;                 // the segment's codes and the end-of-block code
  const int dyn = (int)((PNG_DYN_HEAD + bits + 3 + 7) >> 3) + 4, stored = 5 + len;
  int out_len;
  if (stored <= dyn) {
    out_len = stored;
    uint8_t* ob = reinterpret_cast<uint8_t*>(s_out);
    if (tid == 0) {
      ob[0] = last ? 1 : 0;
      ob[1] = (uint8_t)(len & 255);
      ob[2] = (uint8_t)(len >> 8);
      ob[3] = (uint8_t)(~len & 255);
      ob[4] = (uint8_t)((~len >> 8) & 255);
    }
    for (int i = tid; i < len; i += PNG_T) {
      const int wd = i >> 2;
      ob[5 + i] = (uint8_t)((s_in[wd + (wd >> 5)] >> (8 * (i & 3))) & 255u);
    }
  } else {
    out_len = dyn;
    if (tid == 0) {                             // canonical codes: the first code of every length
      unsigned code = 0;
      s_next[0] = 0;
      for (int l = 1; l < 16; ++l) {
        code = (code + (l > 1 ? s_blc[l - 1] : 0u)) << 1;
        s_next[l] = code;
      }
      png_put(s_out, 0, (2u << 1) | (15u << 13), 17);      // BFINAL 0, BTYPE 10, HLIT 0, HDIST 0, HCLEN 15
    }
    if (tid >= 3 && tid < 19) png_put(s_out, 17 + 3 * tid, 4u, 3);       // code-length code: 4 bits for 0..15
    __syncthreads();
    for (int sym = tid; sym < 257; sym += PNG_T) {
      const unsigned l = s_len[sym];
      unsigned packed = 0;
      if (l) {
        unsigned code = s_next[l];
        for (int q = 0; q < sym; ++q) code += s_len[q] == l ? 1u : 0u;
        packed = (__brev(code) >> (32 - l)) | (l << 16);   // codes go MSB first into an LSB-first stream
      }
      s_code[sym] = packed;
      png_put(s_out, 17 + 57 + 4 * sym, __brev(l) >> 28, 4);
    }                                           // (the one distance length is 0: nothing to set)
    __syncthreads();
    unsigned mine = 0;
    for (int j = 0; j < bn; ++j) mine += s_code[(s_in[33 * tid + (j >> 2)] >> (8 * (j & 3))) & 255u] >> 16;
    s_scan[tid] = mine;
    __syncthreads();
    for (int d = 1; d < PNG_T; d <<= 1) {
      const unsigned add = tid >= d ? s_scan[tid - d] : 0u;
      __syncthreads();
      s_scan[tid] += add;
      __syncthreads();
    }
    unsigned pos = PNG_DYN_HEAD + s_scan[tid] - mine;
    if (bn) {
      unsigned wd = pos >> 5, nb = pos & 31;
      unsigned long long acc = 0;
      for (int j = 0; j < bn; ++j) {
        const unsigned e = s_code[(s_in[33 * tid + (j >> 2)] >> (8 * (j & 3))) & 255u];
        acc |= (unsigned long long)(e & 0xFFFFu) << nb;
        nb += e >> 16;
        if (nb >= 32) {
          atomicOr(&s_out[wd++], (unsigned)acc);
          acc >>= 32;
          nb -= 32;
        }
      }
      if (nb) atomicOr(&s_out[wd], (unsigned)acc);
    }
    if (tid == 0) {
      const unsigned eob = s_code[256], end = PNG_DYN_HEAD + bits;
      png_put(s_out, end - (eob >> 16), eob & 0xFFFFu, (int)(eob >> 16));
      png_put(s_out, end, last ? 1u : 0u, 3);              // the empty stored block: BFINAL, BTYPE 00, pad,
      png_put(s_out, 8u * (unsigned)(dyn - 4) + 16u, 0xFFFFu, 16);       // 00 00 FF FF
    }
  }
  __syncthreads();
  const long long idx = k * nseg + s;
  unsigned* dst = reinterpret_cast<unsigned*>(stage + idx * PNG_STAGE);
  for (int wd = tid; wd < (out_len + 3) >> 2; wd += PNG_T) dst[wd] = s_out[wd];
  if (tid == 0) {
    m_len[idx] = (unsigned)out_len;
    m_s1[idx] = s_s1 % PNG_ADLER;
    m_s2[idx] = (unsigned)(s_s2 % PNG_ADLER);
  }
}

// ---- CRC-32 (reflected, as zlib's): polynomials mod P with x^0 at bit 31 --------------------------------------------
__device__ __forceinline__ unsigned crc_mul(unsigned a, unsigned b) {
  unsigned p = 0;
  for (int i = 0; i < 32; ++i) {
    if (a & (0x80000000u >> i)) p ^= b;
    b = (b >> 1) ^ ((b & 1u) ? CRC_POLY : 0u);
  }
  return p;
}
__device__ __forceinline__ unsigned crc_xpow8(unsigned long long n) {     // x^(8 n) mod P
  unsigned p = 0x80000000u, base = 0x00800000u;
  for (; n; n >>= 1) {
    if (n & 1) p = crc_mul(base, p);
    base = crc_mul(base, base);
  }
  return p;
}
__device__ __forceinline__ unsigned crc_table_entry(int i) {
  unsigned c = (unsigned)i;
  for (int j = 0; j < 8; ++j) c = (c >> 1) ^ ((c & 1u) ? CRC_POLY : 0u);
  return c;
}

__global__ __launch_bounds__(PNG_T) void png_place_kernel(const uint8_t* __restrict__ stage, int nseg,
                                                          const unsigned* __restrict__ m_len,
                                                          unsigned* __restrict__ m_crc, uint8_t* __restrict__ out,
                                                          long long out_stride) {
  __shared__ unsigned s_buf[33 * PNG_T];        // thread t's piece is words 33 t .. 33 t + 32
  __shared__ unsigned s_tab[256];
  __shared__ unsigned long long s_before, s_total;
  __shared__ unsigned s_crc;
  const int s = blockIdx.x, tid = threadIdx.x;
  const long long k = blockIdx.y, idx = k * nseg + s;
  const unsigned* lens = m_len + k * nseg;
  if (tid == 0) { s_before = 0; s_total = 0; s_crc = 0; }
  s_tab[tid] = crc_table_entry(tid);
  __syncthreads();
  unsigned long long before = 0, total = 0;
  for (int j = tid; j < nseg; j += PNG_T) {
    const unsigned l = lens[j];
    total += l;
    if (j < s) before += l;
  }
  atomicAdd(&s_before, before);
  atomicAdd(&s_total, total);
  const int len = (int)lens[s];
  const unsigned* src = reinterpret_cast<const unsigned*>(stage + idx * PNG_STAGE);
  for (int wd = tid; wd < (len + 3) >> 2; wd += PNG_T) s_buf[wd] = src[wd];
  __syncthreads();
  uint8_t* dst = out + k * out_stride + PNG_DATA_AT + (long long)s_before;
  for (int i = tid; i < len; i += PNG_T) dst[i] = (uint8_t)((s_buf[i >> 2] >> (8 * (i & 3))) & 255u);
  const int b0 = 132 * tid, bn = len - b0 < 132 ? (len - b0 < 0 ? 0 : len - b0) : 132;
  if (bn) {
    unsigned c = 0;
    for (int j = 0; j < bn; ++j) {
      const unsigned v = (s_buf[33 * tid + (j >> 2)] >> (8 * (j & 3))) & 255u;
      c = s_tab[(c ^ v) & 255u] ^ (c >> 8);
    }
    // bytes of the IDAT behind this piece: the rest of the segment, the later segments, the Adler-32
    const unsigned long long behind = (unsigned long long)(len - b0 - bn) + (s_total - s_before - (unsigned)len) + 4;
    atomicXor(&s_crc, crc_mul(crc_xpow8(behind), c));
  }
  __syncthreads();
  if (tid == 0) m_crc[idx] = s_crc;
}

__device__ __forceinline__ void png_be32(uint8_t* p, unsigned v) {
  p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)((v >> 16) & 255u); p[2] = (uint8_t)((v >> 8) & 255u); p[3] = (uint8_t)(v & 255u);
}
__device__ __forceinline__ unsigned png_crc_bytes(const unsigned* tab, unsigned c, const uint8_t* p, int n) {
  for (int i = 0; i < n; ++i) c = tab[(c ^ p[i]) & 255u] ^ (c >> 8);
  return c;
}

__global__ __launch_bounds__(PNG_T) void png_finish_kernel(int nseg, int h, int w, const unsigned* __restrict__ m_len,
                                                           const unsigned* __restrict__ m_s1,
                                                           const unsigned* __restrict__ m_s2,
                                                           const unsigned* __restrict__ m_crc,
                                                           const long long flen, uint8_t* __restrict__ out,
                                                           long long out_stride, long long* __restrict__ sizes) {
  __shared__ unsigned s_tab[256];
  __shared__ unsigned long long s_total;
  __shared__ unsigned s_crc;
  __shared__ unsigned long long s_pa[PNG_T], s_pb[PNG_T], s_pl[PNG_T];   // per thread: sum S1, B, raw bytes
  const int tid = threadIdx.x;
  const long long k = blockIdx.x;
  const unsigned *lens = m_len + k * nseg, *s1 = m_s1 + k * nseg, *s2 = m_s2 + k * nseg, *crcs = m_crc + k * nseg;
  if (tid == 0) { s_total = 0; s_crc = 0; }
  s_tab[tid] = crc_table_entry(tid);
  __syncthreads();
  unsigned long long total = 0;
  unsigned x = 0;
  for (int j = tid; j < nseg; j += PNG_T) {
    total += lens[j];
    x ^= crcs[j];
  }
  atomicAdd(&s_total, total);
  atomicXor(&s_crc, x);
  // Adler-32 over a run of consecutive segments, from a = 0: a += S1, b += raw * a_before + S2 (mod 65521)
  const int per = (nseg + PNG_T - 1) / PNG_T, j0 = tid * per, j1 = j0 + per < nseg ? j0 + per : nseg;
  unsigned long long a = 0, b = 0, raw_sum = 0;
  for (int j = j0; j < j1; ++j) {
    const unsigned long long raw = flen - (long long)j * PNG_SEG < PNG_SEG ? flen - (long long)j * PNG_SEG : PNG_SEG;
    b = (b + raw * a + s2[j]) % PNG_ADLER;
    a = (a + s1[j]) % PNG_ADLER;
    raw_sum += raw;
  }
  s_pa[tid] = a; s_pb[tid] = b; s_pl[tid] = raw_sum;
  __syncthreads();
  if (tid != 0) return;
  a = 1; b = 0;
  for (int t = 0; t < PNG_T; ++t) {
    b = (b + (s_pl[t] % PNG_ADLER) * a + s_pb[t]) % PNG_ADLER;
    a = (a + s_pa[t]) % PNG_ADLER;
  }
  const unsigned adler = (unsigned)((b << 16) | a);
  const unsigned long long data = s_total, idat = data + 6;
  uint8_t* o = out + k * out_stride;
  const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
  for (int i = 0; i < 8; ++i) o[i] = sig[i];
  png_be32(o + 8, 13u);
  o[12] = 'I'; o[13] = 'H'; o[14] = 'D'; o[15] = 'R';
  png_be32(o + 16, (unsigned)w);
  png_be32(o + 20, (unsigned)h);
  o[24] = 8; o[25] = 2; o[26] = 0; o[27] = 0; o[28] = 0;
  png_be32(o + 29, ~png_crc_bytes(s_tab, 0xFFFFFFFFu, o + 12, 17));
  png_be32(o + 33, (unsigned)idat);
  o[37] = 'I'; o[38] = 'D'; o[39] = 'A'; o[40] = 'T'; o[41] = 0x78; o[42] = 0x01;
  uint8_t* t = o + PNG_DATA_AT + data;
  png_be32(t, adler);
  // register after `IDAT 78 01` times x^(8 * what follows), the segments' terms, the Adler bytes from a zero register
  unsigned c = png_crc_bytes(s_tab, 0xFFFFFFFFu, o + 37, 6);
  c = crc_mul(crc_xpow8(data + 4), c) ^ s_crc ^ png_crc_bytes(s_tab, 0u, t, 4);
  png_be32(t + 4, ~c);
  png_be32(t + 8, 0u);
  t[12] = 'I'; t[13] = 'E'; t[14] = 'N'; t[15] = 'D';
  png_be32(t + 16, 0xAE426082u);
  sizes[k] = (long long)(PNG_DATA_AT + data + 20);
}

// ---- LZ77 inside a segment (the specification is tests/png_lz_ref.py) -------------------------
// Four more launches between png_segment_kernel and png_place_kernel, a workgroup per segment each, ordered by the
// stream alone; every loop bound is the format's (4 candidates, 258 bytes, 15 doubling rounds, the halving loop):
//   png_lz_sort_kernel   hash << 15 | position of every position with four bytes, bitonic-sorted in LDS: a stable
//                        sort by hash as a plain integer sort
//   png_lz_match_kernel  per sorted rank the up to four predecessors of its hash run, compared a word at a time
//                        against the segment in LDS; length << 16 | distance per position
//   png_lz_parse_kernel  next[i] doubled 15 times, the positions reachable from 0 marked, compacted into tokens
//   png_lz_emit_kernel   the two histograms, the two trees, the block's size; where it beats what
//                        png_segment_kernel staged, the block is written over it and the length replaced
constexpr int PNG_LZ_T = 1024;
constexpr int PNG_LZ_SORT_LDS = PNG_SEG * 4;
constexpr int PNG_LZ_NEXT = PNG_SEG + 8;                                    // next[0 .. len], as 16-bit values
constexpr int PNG_LZ_PARSE_LDS = 2 * PNG_LZ_NEXT * 2;
constexpr int PNG_LZ_IN_WORDS = PNG_SEG / 4 + 4;                            // the segment and 16 bytes of zeros
constexpr int PNG_LZ_LIT = 286, PNG_LZ_DIST = 30, PNG_LZ_SYMS = 288;
constexpr unsigned PNG_LZ_MATCH = 0x80000000u;                              // a token: this | length << 16 | distance

struct png_lz_ws {
  unsigned *keys, *mm, *ntok;                   // n x nseg x PNG_SEG sorted keys, later the tokens; matches; counts
};

static long long png_lz_ws_layout(int n, int h, int w, uint8_t* base, png_ws* ws, png_lz_ws* lz) {
  long long off = png_ws_layout(n, h, w, base, ws) - 16;
  uint8_t* p = reinterpret_cast<uint8_t*>(((uintptr_t)base + 15) & ~(uintptr_t)15);
  const long long per = 4LL * n * ws->nseg * PNG_SEG;
  lz->keys = reinterpret_cast<unsigned*>(p + off); off += per;
  lz->mm = reinterpret_cast<unsigned*>(p + off);   off += per;
  lz->ntok = reinterpret_cast<unsigned*>(p + off); off += round16(4LL * n * ws->nseg);
  return off + 16;
}

__device__ __forceinline__ int png_seg_len(long long flen, int s) {
  const long long rest = flen - (long long)s * PNG_SEG;
  return (int)(rest < PNG_SEG ? rest : PNG_SEG);
}
__device__ __forceinline__ int png_lz_sort_n(int len) {                     // keys sorted: a power of two >= len
  int n = 2;
  while (n < len) n <<= 1;
  return n;
}

__global__ __launch_bounds__(PNG_LZ_T) void png_lz_sort_kernel(const uint8_t* __restrict__ filt, long long fpad,
                                                               long long flen, int nseg, unsigned* __restrict__ keys) {
  extern __shared__ __attribute__((aligned(16))) unsigned png_smem[];
  unsigned* s_k = png_smem;
  const int s = blockIdx.x, tid = threadIdx.x;
  const long long k = blockIdx.y;
  const int len = png_seg_len(flen, s), n = png_lz_sort_n(len);
  const uint8_t* src = filt + k * fpad + (long long)s * PNG_SEG;
  for (int i = tid; i < n; i += PNG_LZ_T) {
    unsigned key = 0xFFFFFFFFu;                 // no four bytes here: behind every key
    if (i + 4 <= len) {
      const unsigned v = (unsigned)src[i] | ((unsigned)src[i + 1] << 8) | ((unsigned)src[i + 2] << 16) |
                         ((unsigned)src[i + 3] << 24);
      key = ((v * 2654435761u) >> 16) << 15 | (unsigned)i;
    }
    s_k[i] = key;
  }
  __syncthreads();
  for (int kk = 2; kk <= n; kk <<= 1)
    for (int j = kk >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (n >> 1); t += PNG_LZ_T) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
        const unsigned a = s_k[i], b = s_k[p];
        if ((a > b) == ((i & kk) == 0)) {
          s_k[i] = b;
          s_k[p] = a;
        }
      }
      __syncthreads();
    }
  unsigned* dst = keys + (k * nseg + s) * PNG_SEG;
  for (int i = tid; i < n; i += PNG_LZ_T) dst[i] = s_k[i];
}

__device__ __forceinline__ unsigned png_ld4(const unsigned* s, int i) {    // the four bytes at byte i of a word array
  const int wd = i >> 2;
  const unsigned long long v = (unsigned long long)s[wd] | ((unsigned long long)s[wd + 1] << 32);
  return (unsigned)(v >> (8 * (i & 3)));
}

__global__ __launch_bounds__(PNG_LZ_T) void png_lz_match_kernel(const uint8_t* __restrict__ filt, long long fpad,
                                                                long long flen, int nseg,
                                                                const unsigned* __restrict__ keys,
                                                                unsigned* __restrict__ mm) {
  __shared__ unsigned s_in[PNG_LZ_IN_WORDS];
  const int s = blockIdx.x, tid = threadIdx.x;
  const long long k = blockIdx.y, idx = k * nseg + s;
  const int len = png_seg_len(flen, s), n = png_lz_sort_n(len), nw = (len + 3) >> 2;
  const unsigned* src = reinterpret_cast<const unsigned*>(filt + k * fpad + (long long)s * PNG_SEG);
  for (int wd = tid; wd < PNG_LZ_IN_WORDS; wd += PNG_LZ_T) {
    unsigned v = wd < nw ? src[wd] : 0u;
    if (wd == nw - 1 && (len & 3)) v &= (1u << (8 * (len & 3))) - 1u;      // bytes past the stream are not data
    s_in[wd] = v;
  }
  __syncthreads();
  const unsigned* sk = keys + idx * PNG_SEG;
  unsigned* out = mm + idx * PNG_SEG;
  if (tid < 3 && len - 1 - tid >= 0) out[len - 1 - tid] = 0u;              // the positions without four bytes
  for (int r = tid; r < n; r += PNG_LZ_T) {
    const unsigned key = sk[r];
    if (key == 0xFFFFFFFFu) continue;
    const int pos = (int)(key & 32767u), cap = len - pos < 258 ? len - pos : 258;
    int best = 0, dist = 0;
    for (int c = 1; c <= 4; ++c) {              // the predecessors in the hash run: earlier positions, nearest first
      if (r - c < 0) break;
      const unsigned kc = sk[r - c];
      if ((kc >> 15) != (key >> 15)) break;
      const int j = (int)(kc & 32767u);
      int l = 0;
      for (; l < cap; l += 4) {                 // at most 65 steps
        const unsigned x = png_ld4(s_in, pos + l) ^ png_ld4(s_in, j + l);
        if (x) {
          l += (__ffs((int)x) - 1) >> 3;
          break;
        }
      }
      l = l < cap ? l : cap;
      if (l > best) {                           // the nearest wins a tie
        best = l;
        dist = pos - j;
      }
    }
    const bool ok = best >= 4 && !(best == 4 && dist > 4096);
    out[pos] = ok ? ((unsigned)best << 16) | (unsigned)dist : 0u;
  }
}

__global__ __launch_bounds__(PNG_LZ_T) void png_lz_parse_kernel(const uint8_t* __restrict__ filt, long long fpad,
                                                                long long flen, int nseg,
                                                                const unsigned* __restrict__ mm,
                                                                unsigned* __restrict__ toks,
                                                                unsigned* __restrict__ m_ntok) {
  extern __shared__ __attribute__((aligned(16))) unsigned png_smem[];
  unsigned short* s_a = reinterpret_cast<unsigned short*>(png_smem);
  unsigned short* s_b = s_a + PNG_LZ_NEXT;
  __shared__ unsigned s_flag[PNG_LZ_T + 1], s_scan[PNG_LZ_T];
  const int s = blockIdx.x, tid = threadIdx.x;
  const long long k = blockIdx.y, idx = k * nseg + s;
  const int len = png_seg_len(flen, s);
  const uint8_t* src = filt + k * fpad + (long long)s * PNG_SEG;
  const unsigned* m = mm + idx * PNG_SEG;
  for (int i = tid; i <= len; i += PNG_LZ_T) {
    int nx = len;
    if (i < len) {
      const unsigned l = m[i] >> 16;
      nx = i + (l ? (int)l : 1);
    }
    s_a[i] = (unsigned short)nx;                // <= len <= 32768
  }
  s_flag[tid] = tid == 0 ? 1u : 0u;
  if (tid == 0) s_flag[PNG_LZ_T] = 0u;
  __syncthreads();
  for (int round = 0; round < 15; ++round) {    // marked: what 0 reaches in less than 2^round steps; next: 2^round steps
    for (int i = tid; i <= len; i += PNG_LZ_T)
      if ((s_flag[i >> 5] >> (i & 31)) & 1u) {
        const int t = s_a[i];
        atomicOr(&s_flag[t >> 5], 1u << (t & 31));
      }
    for (int i = tid; i <= len; i += PNG_LZ_T) s_b[i] = s_a[s_a[i]];
    __syncthreads();
    unsigned short* sw = s_a; s_a = s_b; s_b = sw;
  }
  unsigned mine = s_flag[tid];                  // positions 32 tid .. 32 tid + 31
  if (32 * tid + 32 > len) mine &= 32 * tid >= len ? 0u : (1u << (len - 32 * tid)) - 1u;
  const unsigned cnt = (unsigned)__popc(mine);
  s_scan[tid] = cnt;
  __syncthreads();
  for (int d = 1; d < PNG_LZ_T; d <<= 1) {
    const unsigned add = tid >= d ? s_scan[tid - d] : 0u;
    __syncthreads();
    s_scan[tid] += add;
    __syncthreads();
  }
  unsigned at = s_scan[tid] - cnt;
  unsigned* dst = toks + idx * PNG_SEG;
  while (mine) {
    const int b = __ffs((int)mine) - 1, pos = 32 * tid + b;
    mine &= mine - 1u;
    const unsigned v = m[pos];
    dst[at++] = v ? (PNG_LZ_MATCH | v) : (unsigned)src[pos];
  }
  if (tid == PNG_LZ_T - 1) m_ntok[idx] = s_scan[tid];
}

// RFC 1951 section 3.2.5 in closed form: (symbol - 257, extra bits, their value) of a length, the same of a distance
__device__ __forceinline__ void png_len_sym(unsigned len, unsigned* sym, unsigned* nb, unsigned* ex) {
  const unsigned x = len - 3u;
  if (len == 258u) { *sym = 28u; *nb = 0u; *ex = 0u; return; }
  if (x < 8u) { *sym = x; *nb = 0u; *ex = 0u; return; }
  const unsigned e = 29u - (unsigned)__clz(x);                            // floor(log2 x) - 2
  *sym = 4u * e + 4u + ((x >> e) & 3u);
  *nb = e;
  *ex = x & ((1u << e) - 1u);
}
__device__ __forceinline__ void png_dist_sym(unsigned dist, unsigned* sym, unsigned* nb, unsigned* ex) {
  const unsigned x = dist - 1u;
  if (x < 4u) { *sym = x; *nb = 0u; *ex = 0u; return; }
  const unsigned lg = 31u - (unsigned)__clz(x);
  *sym = 2u * lg + ((x >> (lg - 1u)) & 1u);
  *nb = lg - 1u;
  *ex = x & ((1u << (lg - 1u)) - 1u);
}

struct png_tree_lds {                           // what one tree construction needs beside counts and lengths
  unsigned wt[PNG_LZ_SYMS], sw[PNG_LZ_SYMS], ss[PNG_LZ_SYMS], pl[PNG_LZ_SYMS], iw[PNG_LZ_SYMS], pi[PNG_LZ_SYMS],
      di[PNG_LZ_SYMS], blc[16], next[16], n, max;
};

// Code lengths and canonical codes of an alphabet of A symbols by png_segment_kernel's rule; code[sym] = the code
// bit-reversed | length << 16.  One used symbol: length 1.  Called by the whole workgroup.
template <int A>
__device__ void png_lz_tree(const unsigned* cnt, unsigned* len, unsigned* code, png_tree_lds* w) {
  const int tid = threadIdx.x;
  for (int sym = tid; sym < A; sym += PNG_T) w->wt[sym] = cnt[sym];
  for (;;) {
    if (tid == 0) { w->n = 0; w->max = 0; }
    __syncthreads();
    for (int sym = tid; sym < A; sym += PNG_T) {
      const unsigned wt = w->wt[sym];
      len[sym] = 0;
      if (wt) {
        unsigned rank = 0;
        for (int q = 0; q < A; ++q) {
          const unsigned wq = w->wt[q];
          rank += (wq != 0 && (wq < wt || (wq == wt && q < sym))) ? 1u : 0u;
        }
        w->sw[rank] = wt;
        w->ss[rank] = (unsigned)sym;
        atomicAdd(&w->n, 1u);
      }
    }
    __syncthreads();
    const int n = (int)w->n;
    if (n == 1) {
      if (tid == 0) len[w->ss[0]] = 1u;
      __syncthreads();
      break;
    }
    if (tid == 0) {
      int li = 0, ii = 0, ni = 0;
      for (int step = 0; step < n - 1; ++step) {
        unsigned wsum = 0;
        for (int q = 0; q < 2; ++q) {
          if (li < n && (ii >= ni || w->sw[li] <= w->iw[ii])) {   // equal weights: the leaf, its id is the lower
            wsum += w->sw[li];
            w->pl[li++] = (unsigned)step;
          } else {
            wsum += w->iw[ii];
            w->pi[ii++] = (unsigned)step;
          }
        }
        w->iw[ni++] = wsum;
      }
      w->di[n - 2] = 0;
      for (int i = n - 3; i >= 0; --i) w->di[i] = w->di[w->pi[i]] + 1;
    }
    __syncthreads();
    for (int i = tid; i < n; i += PNG_T) {
      const unsigned l = w->di[w->pl[i]] + 1;
      len[w->ss[i]] = l;
      atomicMax(&w->max, l);
    }
    __syncthreads();
    const unsigned mx = w->max;
    __syncthreads();
    if (mx <= 15) break;
    for (int sym = tid; sym < A; sym += PNG_T) {
      const unsigned wt = w->wt[sym];
      w->wt[sym] = wt ? (wt + 1) >> 1 : 0;
    }
  }
  if (tid < 16) w->blc[tid] = 0;
  __syncthreads();
  for (int sym = tid; sym < A; sym += PNG_T)
    if (len[sym]) atomicAdd(&w->blc[len[sym]], 1u);
  __syncthreads();
  if (tid == 0) {
    unsigned c = 0;
    w->next[0] = 0;
    for (int l = 1; l < 16; ++l) {
      c = (c + (l > 1 ? w->blc[l - 1] : 0u)) << 1;
      w->next[l] = c;
    }
  }
  __syncthreads();
  for (int sym = tid; sym < A; sym += PNG_T) {
    const unsigned l = len[sym];
    unsigned packed = 0;
    if (l) {
      unsigned c = w->next[l];
      for (int q = 0; q < sym; ++q) c += len[q] == l ? 1u : 0u;
      packed = (__brev(c) >> (32 - l)) | (l << 16);
    }
    code[sym] = packed;
  }
  __syncthreads();
}

// (bits, their count) of a token's literal or length part and of its distance part (count 0 for a literal)
__device__ __forceinline__ void png_lz_token_bits(unsigned tok, const unsigned* lcode, const unsigned* dcode,
                                                  unsigned* v0, unsigned* n0, unsigned* v1, unsigned* n1) {
  if (tok & PNG_LZ_MATCH) {
    unsigned sym, nb, ex;
    png_len_sym((tok >> 16) & 511u, &sym, &nb, &ex);
    const unsigned lc = lcode[257u + sym];
    *v0 = (lc & 0xFFFFu) | (ex << (lc >> 16));
    *n0 = (lc >> 16) + nb;
    png_dist_sym(tok & 0xFFFFu, &sym, &nb, &ex);
    const unsigned dc = dcode[sym];
    *v1 = (dc & 0xFFFFu) | (ex << (dc >> 16));
    *n1 = (dc >> 16) + nb;
  } else {
    const unsigned lc = lcode[tok];
    *v0 = lc & 0xFFFFu;
    *n0 = lc >> 16;
    *v1 = 0u;
    *n1 = 0u;
  }
}

__global__ __launch_bounds__(PNG_T) void png_lz_emit_kernel(long long flen, int nseg, const unsigned* __restrict__ toks,
                                                            const unsigned* __restrict__ m_ntok,
                                                            uint8_t* __restrict__ stage, unsigned* __restrict__ m_len) {
  __shared__ unsigned s_out[PNG_OUT_WORDS];
  __shared__ unsigned s_lcnt[PNG_LZ_SYMS], s_llen[PNG_LZ_SYMS], s_lcode[PNG_LZ_SYMS];
  __shared__ unsigned s_dcnt[32], s_dlen[32], s_dcode[32], s_scan[PNG_T];
  __shared__ png_tree_lds s_tree;
  __shared__ unsigned s_nm, s_bits, s_hl, s_hd;
  const int s = blockIdx.x, tid = threadIdx.x;
  const long long k = blockIdx.y, idx = k * nseg + s;
  const bool last = s == nseg - 1;
  const unsigned* tok = toks + idx * PNG_SEG;
  const int ntok = (int)m_ntok[idx];
  for (int i = tid; i < PNG_LZ_SYMS; i += PNG_T) s_lcnt[i] = 0u;
  if (tid < 32) s_dcnt[tid] = 0u;
  if (tid == 0) { s_nm = 0; s_bits = 0; s_hl = 256; s_hd = 0; }
  __syncthreads();
  {
    unsigned nm = 0;
    for (int t = tid; t < ntok; t += PNG_T) {
      const unsigned v = tok[t];
      if (v & PNG_LZ_MATCH) {
        unsigned sym, nb, ex;
        png_len_sym((v >> 16) & 511u, &sym, &nb, &ex);
        atomicAdd(&s_lcnt[257u + sym], 1u);
        png_dist_sym(v & 0xFFFFu, &sym, &nb, &ex);
        atomicAdd(&s_dcnt[sym], 1u);
        ++nm;
      } else {
        atomicAdd(&s_lcnt[v], 1u);
      }
    }
    if (nm) atomicAdd(&s_nm, nm);
  }
  if (tid == 0) s_lcnt[256] = 1u;
  __syncthreads();
  if (s_nm == 0) return;                        // no match: no LZ candidate
  png_lz_tree<PNG_LZ_LIT>(s_lcnt, s_llen, s_lcode, &s_tree);
  png_lz_tree<PNG_LZ_DIST>(s_dcnt, s_dlen, s_dcode, &s_tree);
  for (int sym = tid; sym < PNG_LZ_LIT; sym += PNG_T) {
    const unsigned c = s_lcnt[sym];
    if (c) {
      unsigned extra = 0;
      if (sym >= 265 && sym < 285) extra = (unsigned)(sym - 261) >> 2;
      atomicAdd(&s_bits, c * (s_llen[sym] + extra));
      atomicMax(&s_hl, (unsigned)sym);
    }
  }
  if (tid < PNG_LZ_DIST && s_dcnt[tid]) {
    atomicAdd(&s_bits, s_dcnt[tid] * (s_dlen[tid] + (tid >= 4 ? (unsigned)(tid - 2) >> 1 : 0u)));
    atomicMax(&s_hd, (unsigned)tid);
  }
  __syncthreads();
  const unsigned nl = s_hl + 1u, nd = s_hd + 1u;                          // HLIT + 257 and HDIST + 1
  const unsigned head = 3u + 14u + 57u + 4u * (nl + nd), bits = s_bits;   // bits: the tokens and the end-of-block code
  const unsigned out_len = ((head + bits + 3u + 7u) >> 3) + 4u;
  if (out_len >= m_len[idx]) return;            // stored or Huffman-only is not larger: it stays
  for (int wd = tid; wd < PNG_OUT_WORDS; wd += PNG_T) s_out[wd] = 0u;
  __syncthreads();
  if (tid == 0) png_put(s_out, 0, (2u << 1) | ((nl - 257u) << 3) | ((nd - 1u) << 8) | (15u << 13), 17);
  if (tid >= 3 && tid < 19) png_put(s_out, 17 + 3 * tid, 4u, 3);          // code-length code: 4 bits for 0..15
  for (unsigned sym = tid; sym < nl + nd; sym += PNG_T) {
    const unsigned l = sym < nl ? s_llen[sym] : s_dlen[sym - nl];
    png_put(s_out, 17 + 57 + 4 * sym, __brev(l) >> 28, 4);
  }
  const int per = (ntok + PNG_T - 1) / PNG_T, t0 = tid * per, t1 = t0 + per < ntok ? t0 + per : ntok;
  unsigned mine = 0;
  for (int t = t0; t < t1; ++t) {
    unsigned v0, n0, v1, n1;
    png_lz_token_bits(tok[t], s_lcode, s_dcode, &v0, &n0, &v1, &n1);
    mine += n0 + n1;
  }
  s_scan[tid] = mine;
  __syncthreads();
  for (int d = 1; d < PNG_T; d <<= 1) {
    const unsigned add = tid >= d ? s_scan[tid - d] : 0u;
    __syncthreads();
    s_scan[tid] += add;
    __syncthreads();
  }
  if (t0 < t1) {
    const unsigned pos = head + s_scan[tid] - mine;
    unsigned wd = pos >> 5, nb = pos & 31;
    unsigned long long acc = 0;
    for (int t = t0; t < t1; ++t) {
      unsigned v[2], nn[2];
      png_lz_token_bits(tok[t], s_lcode, s_dcode, &v[0], &nn[0], &v[1], &nn[1]);
      for (int q = 0; q < 2; ++q) {             // at most 20 and 28 bits behind fewer than 32: whole-word shifts
        acc |= (unsigned long long)v[q] << nb;
        nb += nn[q];
        if (nb >= 32) {
          atomicOr(&s_out[wd++], (unsigned)acc);
          acc >>= 32;
          nb -= 32;
        }
      }
    }
    if (nb) atomicOr(&s_out[wd], (unsigned)acc);
  }
  if (tid == 0) {
    const unsigned eob = s_lcode[256], end = head + bits;
    png_put(s_out, end - (eob >> 16), eob & 0xFFFFu, (int)(eob >> 16));
    png_put(s_out, end, last ? 1u : 0u, 3);                // the empty stored block: BFINAL, BTYPE 00, pad,
    png_put(s_out, 8u * (out_len - 4u) + 16u, 0xFFFFu, 16);               // 00 00 FF FF
  }
  __syncthreads();
  unsigned* dst = reinterpret_cast<unsigned*>(stage + idx * PNG_STAGE);
  for (int wd = tid; wd < (int)((out_len + 3u) >> 2); wd += PNG_T) dst[wd] = s_out[wd];
  if (tid == 0) m_len[idx] = out_len;
}

static int png_check_shape(const char* what, int h, int w) {
  TG_REQUIRE(h >= 1 && w >= 1, TG_E_ARG, "%s: h=%d w=%d (h, w >= 1)", what, h, w);
  TG_REQUIRE(png_flen(h, w) < (1LL << 31), TG_E_SHAPE, "%s: h=%d w=%d: the filtered stream h * (3 w + 1) = %lld is 2^31 bytes or more",
             what, h, w, png_flen(h, w));
  return TG_OK;
}

}  // namespace tg

extern "C" int64_t tg_png_capacity(int h, int w) {
  if (tg::png_check_shape("png_capacity", h, w) != TG_OK) return -1;
  const long long flen = tg::png_flen(h, w);
  return tg::PNG_DATA_AT + 20 + flen + 5 * tg::png_nseg(flen);
}

extern "C" int64_t tg_png_workspace_bytes(int n, int h, int w) {
  if (tg::png_check_shape("png_workspace_bytes", h, w) != TG_OK) return -1;
  if (n < 1 || n > 65535) {
    tg::set_error("png_workspace_bytes: n=%d (1 <= n <= 65535)", n);
    return -1;
  }
  tg::png_ws ws;
  return tg::png_ws_layout(n, h, w, nullptr, &ws);
}

extern "C" int tg_png_encode_u8(const uint8_t* rgb_hwc, int n, int h, int w, int filter, uint8_t* out,
                                int64_t out_stride, int64_t* sizes, void* workspace, tg_stream_t stream) {
  TG_REQUIRE(rgb_hwc && out && sizes && workspace, TG_E_ARG, "png_encode_u8: null pointer");
  TG_REQUIRE(n >= 1 && n <= 65535, TG_E_ARG, "png_encode_u8: n=%d (1 <= n <= 65535)", n);
  TG_REQUIRE(filter == TG_PNG_FILTER_NONE || filter == TG_PNG_FILTER_ADAPTIVE, TG_E_ARG, "png_encode_u8: filter=%d", filter);
  const int rc = tg::png_check_shape("png_encode_u8", h, w);
  if (rc != TG_OK) return rc;
  TG_REQUIRE(out_stride >= tg_png_capacity(h, w), TG_E_SHAPE,
             "png_encode_u8: out_stride=%lld is less than the %lld bytes a %dx%d frame can need (tg_png_capacity)",
             (long long)out_stride, (long long)tg_png_capacity(h, w), h, w);
  TG_REQUIRE((uintptr_t)sizes % 8 == 0, TG_E_ARG, "png_encode_u8: sizes is not 8-byte aligned");
  tg::png_ws ws;
  tg::png_ws_layout(n, h, w, static_cast<uint8_t*>(workspace), &ws);
  if (const int rc = tg::ensure_dynamic_lds<tg::png_segment_kernel>(tg::PNG_SEG_LDS, "png_segment")) return rc;
  const hipStream_t st = (hipStream_t)stream;
  const dim3 block(tg::PNG_T), rows((unsigned)h, (unsigned)n), segs((unsigned)ws.nseg, (unsigned)n);
  if (filter == TG_PNG_FILTER_ADAPTIVE)
    hipLaunchKernelGGL(tg::png_filter_kernel<true>, rows, block, 0, st, rgb_hwc, ws.filt, h, w, ws.fpad);
  else
    hipLaunchKernelGGL(tg::png_filter_kernel<false>, rows, block, 0, st, rgb_hwc, ws.filt, h, w, ws.fpad);
  hipLaunchKernelGGL(tg::png_segment_kernel, segs, block, tg::PNG_SEG_LDS, st, ws.filt, ws.fpad, ws.flen, ws.nseg,
                     ws.stage, ws.len, ws.s1, ws.s2);
  hipLaunchKernelGGL(tg::png_place_kernel, segs, block, 0, st, ws.stage, ws.nseg, ws.len, ws.crc, out,
                     (long long)out_stride);
  hipLaunchKernelGGL(tg::png_finish_kernel, dim3((unsigned)n), block, 0, st, ws.nseg, h, w, ws.len, ws.s1, ws.s2, ws.crc,
                     ws.flen, out, (long long)out_stride, reinterpret_cast<long long*>(sizes));
  return tg::check_launch("png_encode_u8");
}

extern "C" int64_t tg_png_lz_workspace_bytes(int n, int h, int w) {
  if (tg::png_check_shape("png_lz_workspace_bytes", h, w) != TG_OK) return -1;
  if (n < 1 || n > 65535) {
    tg::set_error("png_lz_workspace_bytes: n=%d (1 <= n <= 65535)", n);
    return -1;
  }
  tg::png_ws ws;
  tg::png_lz_ws lz;
  return tg::png_lz_ws_layout(n, h, w, nullptr, &ws, &lz);
}

extern "C" int tg_png_encode_lz_u8(const uint8_t* rgb_hwc, int n, int h, int w, int filter, uint8_t* out,
                                   int64_t out_stride, int64_t* sizes, void* workspace, tg_stream_t stream) {
  TG_REQUIRE(rgb_hwc && out && sizes && workspace, TG_E_ARG, "png_encode_lz_u8: null pointer");
  TG_REQUIRE(n >= 1 && n <= 65535, TG_E_ARG, "png_encode_lz_u8: n=%d (1 <= n <= 65535)", n);
  TG_REQUIRE(filter == TG_PNG_FILTER_NONE || filter == TG_PNG_FILTER_ADAPTIVE, TG_E_ARG, "png_encode_lz_u8: filter=%d", filter);
  const int rc = tg::png_check_shape("png_encode_lz_u8", h, w);
  if (rc != TG_OK) return rc;
  TG_REQUIRE(out_stride >= tg_png_capacity(h, w), TG_E_SHAPE,
             "png_encode_lz_u8: out_stride=%lld is less than the %lld bytes a %dx%d frame can need (tg_png_capacity)",
             (long long)out_stride, (long long)tg_png_capacity(h, w), h, w);
  TG_REQUIRE((uintptr_t)sizes % 8 == 0, TG_E_ARG, "png_encode_lz_u8: sizes is not 8-byte aligned");
  tg::png_ws ws;
  tg::png_lz_ws lz;
  tg::png_lz_ws_layout(n, h, w, static_cast<uint8_t*>(workspace), &ws, &lz);
  if (const int rc = tg::ensure_dynamic_lds<tg::png_segment_kernel>(tg::PNG_SEG_LDS, "png_segment")) return rc;
  if (const int rc = tg::ensure_dynamic_lds<tg::png_lz_sort_kernel>(tg::PNG_LZ_SORT_LDS, "png_lz_sort")) return rc;
  if (const int rc = tg::ensure_dynamic_lds<tg::png_lz_parse_kernel>(tg::PNG_LZ_PARSE_LDS, "png_lz_parse")) return rc;
  const hipStream_t st = (hipStream_t)stream;
  const dim3 block(tg::PNG_T), wide(tg::PNG_LZ_T), rows((unsigned)h, (unsigned)n), segs((unsigned)ws.nseg, (unsigned)n);
  if (filter == TG_PNG_FILTER_ADAPTIVE)
    hipLaunchKernelGGL(tg::png_filter_kernel<true>, rows, block, 0, st, rgb_hwc, ws.filt, h, w, ws.fpad);
  else
    hipLaunchKernelGGL(tg::png_filter_kernel<false>, rows, block, 0, st, rgb_hwc, ws.filt, h, w, ws.fpad);
  hipLaunchKernelGGL(tg::png_segment_kernel, segs, block, tg::PNG_SEG_LDS, st, ws.filt, ws.fpad, ws.flen, ws.nseg,
                     ws.stage, ws.len, ws.s1, ws.s2);
  hipLaunchKernelGGL(tg::png_lz_sort_kernel, segs, wide, tg::PNG_LZ_SORT_LDS, st, ws.filt, ws.fpad, ws.flen, ws.nseg,
                     lz.keys);
  hipLaunchKernelGGL(tg::png_lz_match_kernel, segs, wide, 0, st, ws.filt, ws.fpad, ws.flen, ws.nseg, lz.keys, lz.mm);
  hipLaunchKernelGGL(tg::png_lz_parse_kernel, segs, wide, tg::PNG_LZ_PARSE_LDS, st, ws.filt, ws.fpad, ws.flen, ws.nseg,
                     lz.mm, lz.keys, lz.ntok);             // (the tokens go where the sorted keys were)
  hipLaunchKernelGGL(tg::png_lz_emit_kernel, segs, block, 0, st, ws.flen, ws.nseg, lz.keys, lz.ntok, ws.stage, ws.len);
  hipLaunchKernelGGL(tg::png_place_kernel, segs, block, 0, st, ws.stage, ws.nseg, ws.len, ws.crc, out,
                     (long long)out_stride);
  hipLaunchKernelGGL(tg::png_finish_kernel, dim3((unsigned)n), block, 0, st, ws.nseg, h, w, ws.len, ws.s1, ws.s2, ws.crc,
                     ws.flen, out, (long long)out_stride, reinterpret_cast<long long*>(sizes));
  return tg::check_launch("png_encode_lz_u8");
}
