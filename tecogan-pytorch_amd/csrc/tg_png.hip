// PNG files of uint8 HWC RGB frames, encoded on the device: what --mode infer writes into a PNG
// folder, without the host's zlib.  The specification is tests/png_ref.py and the bytes must be equal: scanline
// filtering per row, the filtered stream cut into segments of 32768 bytes, every segment deflated on its own with
// Huffman codes only (one dynamic block plus an empty stored block for byte alignment, or one stored block when that
// is not larger), one IDAT.  No LZ77 matches: file size is the price.
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
  static bool lds_ok = false;
  if (!lds_ok) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(tg::png_segment_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, tg::PNG_SEG_LDS);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      tg::set_error("png_encode_u8: %d bytes of LDS per workgroup: %s", tg::PNG_SEG_LDS, hipGetErrorString(e));
      return TG_E_HIP;
    }
    lds_ok = true;
  }
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
