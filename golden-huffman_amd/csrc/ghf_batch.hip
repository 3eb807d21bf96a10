// golden-huffman_amd/csrc/ghf_batch.hip -- many small independent .crs2 streams in one launch per direction
// (ghf_compress_batch / ghf_decode_batch, include/ghf.h).
//
// One workgroup owns one item from its first byte to its last, so nothing crosses a workgroup: no workspace scans, no
// 16-byte unit with two writers, no atomics to memory and no pre-zeroed output.  What the single-stream path spreads
// over five launches (K1, K2+K3, K4, K5 and the header) happens inside the workgroup; the one-wavefront code build, which
// costs a looping caller 0.26 ms per item on an idle GPU, is hidden by the other workgroups resident on the same CU.
#include "ghf_build_code.h"

namespace ghf {

constexpr int kBatchThreads = 256;
constexpr int kBatchWaves = kBatchThreads / kWave;
// a round = one side-car block: 256 lanes x 16 symbols; four lanes share a 64-symbol segment, as in K5
constexpr int kBatchRoundSymbols = kBatchThreads * kSymPerLane;
static_assert(kBatchRoundSymbols == kBlockSymbols, "a round of k_compress_batch is one side-car block");
// the packed bits of a round: up to 127 carried bits + 4096 codes of <= 32 bits + end mark + padding
constexpr int kBatchStageWords = kBatchRoundSymbols + 8;

// ---- the item's bytes ------------------------------------------------------------------------------------------------
// in[off .. off + 16) as four little-endian words, for any alignment of `in` (off is a multiple of 16, off < n).  Whole
// vectors come from one aligned 16-byte load, or from the two aligned vectors that hold them (the bytes in front of
// in[0] that this touches share a 16-byte granule with in[0]); the item's ragged end is read byte by byte.
__device__ __forceinline__ uint4 batch_load16(const uint8_t* __restrict__ in, uint32_t off, uint32_t n, uint32_t mis) {
  const uint8_t* p = in + off;
  if (off + 16u <= n) {
    if (mis == 0) return *reinterpret_cast<const uint4*>(p);
    const uint4 a = *reinterpret_cast<const uint4*>(p - mis);
    const uint4 b = *reinterpret_cast<const uint4*>(p - mis + 16);
    uint32_t w0 = a.x, w1 = a.y, w2 = a.z, w3 = a.w, w4 = b.x, w5 = b.y, w6 = b.z, w7 = b.w;
    if (mis & 4u) { w0 = w1; w1 = w2; w2 = w3; w3 = w4; w4 = w5; w5 = w6; w6 = w7; }
    if (mis & 8u) { w0 = w2; w1 = w3; w2 = w4; w3 = w5; w4 = w6; }
    const uint32_t sh = 8u * (mis & 3u);
    return make_uint4(alignbit(w1, w0, sh), alignbit(w2, w1, sh), alignbit(w3, w2, sh), alignbit(w4, w3, sh));
  }
  uint32_t q0 = 0, q1 = 0, q2 = 0, q3 = 0;
#pragma unroll
  for (uint32_t j = 0; j < 16; ++j) {
    if (off + j < n) {
      const uint32_t b = (uint32_t)p[j] << (8 * (j & 3));
      if (j < 4) q0 |= b;
      else if (j < 8) q1 |= b;
      else if (j < 12) q2 |= b;
      else q3 |= b;
    }
  }
  return make_uint4(q0, q1, q2, q3);
}

__device__ __forceinline__ uint32_t batch_byte(const uint4& v, int k) {
  const uint32_t w = k < 4 ? v.x : k < 8 ? v.y : k < 12 ? v.z : v.w;
  return (w >> (8 * (k & 3))) & 0xFFu;
}

struct LdsCounts {  // the workgroup's 256 byte counts; the end mark counts once (include/encoder.h:123-129)
  const uint32_t* bins;
  __device__ __forceinline__ long long operator()(int s) const { return s < 256 ? (long long)bins[s] : 1ll; }
};

struct BatchCompressLds {
  HeapLds heap;
  CodeLds cl;
  uint32_t bins[kBatchWaves][256];  // one replica per wave; summed into bins[0]
  uint2 tab[GHF_NSYM + 3];          // (length, codeword)
  alignas(16) uint32_t stage[kBatchStageWords];  // the round's bits, MSB first; word w = stream bits [32 w, 32 w + 32) of the stage
  uint32_t wave_bits[kBatchWaves];
  unsigned long long body_bits;
  int ndata;
  int status;
};
static_assert(sizeof(BatchCompressLds) <= 32 * 1024, "five workgroups per CU");

// `len` bits (1..32) of `cw` at stage bit `pos`
__device__ __forceinline__ void stage_put(uint32_t* stage, uint32_t pos, uint32_t len, uint32_t cw) {
  const uint32_t w = pos >> 5, o = pos & 31u;
  const unsigned long long v = (unsigned long long)cw << (64u - o - len);
  atomicOr(&stage[w], (uint32_t)(v >> 32));
  if (o + len > 32u) atomicOr(&stage[w + 1], (uint32_t)v);
}

__global__ __launch_bounds__(kBatchThreads) void k_compress_batch(BatchCompressParams P) {
  __shared__ BatchCompressLds S;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t item = blockIdx.x;
  const uint64_t n64 = P.in_bytes[item];
  const uint8_t* __restrict__ const in = P.in_ptrs[item];
  uint8_t* __restrict__ const out = P.out_ptrs[item];
  const uint64_t cap = P.out_caps[item];
  int refuse = GHF_OK;
  if (n64 == 0) refuse = GHF_E_EMPTY;
  else if (n64 > P.max_item_bytes || !in || !out || (reinterpret_cast<uintptr_t>(out) & 15u)) refuse = GHF_E_INVAL;
  if (refuse) {
    if (tid == 0) {
      P.item_status[item] = refuse;
      P.out_bytes[item] = 0;
    }
    return;
  }
  const uint32_t n = (uint32_t)n64;
  const uint32_t mis = (uint32_t)reinterpret_cast<uintptr_t>(in) & 15u;
  ghf_code* const code = P.codes + item;

  // ---- K1: byte counts ----
  for (int i = tid; i < kBatchWaves * 256; i += kBatchThreads) (&S.bins[0][0])[i] = 0;
  if (tid == 0) {
    S.status = 0;
    S.body_bits = 0;
  }
  __syncthreads();
  for (uint32_t off = (uint32_t)tid * 16u; off < n; off += kBatchRoundSymbols) {
    const uint4 v = batch_load16(in, off, n, mis);
    const uint32_t cnt = n - off < 16u ? n - off : 16u;
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if ((uint32_t)k < cnt) atomicAdd(&S.bins[wave][batch_byte(v, k)], 1u);
  }
  __syncthreads();
  {
    uint32_t c = 0;
#pragma unroll
    for (int w = 0; w < kBatchWaves; ++w) c += S.bins[w][tid];
    __syncthreads();
    S.bins[0][tid] = c;
  }
  __syncthreads();

  // ---- K2 + K3 on wave 0, the same body k_build_code runs; the tables go to codes[item] ----
  if (wave == 0) {
    NoLimitLds q;
    build_code_body<false, false>(S.heap, q, S.cl, S.ndata, LdsCounts{S.bins[0]}, code, &S.status, 0u, lane);
  }
  __syncthreads();
  if (S.status != 0) {  // (GHF_E_CODELEN needs far more than 1 MiB; kept for completeness)
    if (tid == 0) {
      P.item_status[item] = S.status;
      P.out_bytes[item] = 0;
    }
    return;
  }
  for (int s = tid; s < GHF_NSYM; s += kBatchThreads) S.tab[s] = make_uint2(code->length[s], code->codeword[s]);
  const int max_len = code->max_len;
  {
    const unsigned long long b = (unsigned long long)S.bins[0][tid] * code->length[tid];
    if (b) atomicAdd(&S.body_bits, b);
  }
  __syncthreads();
  const uint32_t end_len = S.tab[GHF_NSYM - 1].x, end_cw = S.tab[GHF_NSYM - 1].y;
  const uint32_t hdr_bytes = 1040u + 8u * (uint32_t)max_len;
  const uint64_t image_bits = 8ull * hdr_bytes + S.body_bits + end_len;
  const uint64_t image_bytes = (image_bits + 7) >> 3;
  if (image_bytes > cap) {
    if (tid == 0) {
      P.item_status[item] = GHF_E_CAP;
      P.out_bytes[item] = 0;
    }
    return;
  }

  // ---- a5: the header's whole 16-byte units; with an odd max_len its last 8 bytes share a unit with the body ----
  const uint32_t hdr_full_words = (hdr_bytes & ~15u) >> 2;
  for (uint32_t w = tid; w < hdr_full_words; w += kBatchThreads)
    reinterpret_cast<uint32_t*>(out)[w] = bswap32(header_word(code, (int)w, max_len));
  for (int w = tid; w < kBatchStageWords; w += kBatchThreads) S.stage[w] = 0;
  uint32_t B = 8u * hdr_bytes;  // image bit of the next code (an item has at most 2^20 codes of <= 32 bits)
  if ((uint32_t)tid < ((B & 127u) >> 5)) S.stage[tid] = header_word(code, (int)(hdr_full_words + tid), max_len);

  uint64_t* const chunk_bit = P.chunk_bit ? P.chunk_bit + (uint64_t)item * P.blocks_per_item : nullptr;
  uint32_t* const seg_bit = P.seg_bit ? P.seg_bit + (uint64_t)item * P.segs_per_item : nullptr;

  // ---- K4 + K5: one side-car block per round ----
  const uint32_t nrounds = (n + kBatchRoundSymbols - 1) / kBatchRoundSymbols;
#pragma unroll 1
  for (uint32_t r = 0; r < nrounds; ++r) {
    const uint32_t off = r * kBatchRoundSymbols + (uint32_t)tid * 16u;
    const uint32_t cnt = off < n ? (n - off < 16u ? n - off : 16u) : 0u;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (cnt) v = batch_load16(in, off, n, mis);
    uint32_t bits = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if ((uint32_t)k < cnt) bits += S.tab[batch_byte(v, k)].x;
    const uint32_t incl = wave_incl_scan_u32(bits);
    if (lane == 63) S.wave_bits[wave] = incl;
    __syncthreads();  // (also: the stage is zeroed and holds the carried bits)
    uint32_t before = 0, round_bits = 0;
#pragma unroll
    for (int w = 0; w < kBatchWaves; ++w) {
      const uint32_t t = S.wave_bits[w];
      before += w < wave ? t : 0u;
      round_bits += t;
    }
    const uint32_t carry = B & 127u;
    const uint32_t seg_end = before + incl;  // relative to the block's first code
    {
      uint32_t pos = carry + seg_end - bits;
      uint32_t w = pos >> 5, nb = pos & 31u;
      unsigned long long acc = 0;
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        if ((uint32_t)k < cnt) {
          const uint2 e = S.tab[batch_byte(v, k)];
          acc |= (unsigned long long)e.y << (64u - nb - e.x);
          nb += e.x;
          if (nb >= 32u) {
            atomicOr(&S.stage[w], (uint32_t)(acc >> 32));
            ++w;
            acc <<= 32;
            nb -= 32u;
          }
        }
      }
      if (cnt && nb) atomicOr(&S.stage[w], (uint32_t)(acc >> 32));
    }
    if (seg_bit && (tid & 3) == 3 && r * kBatchRoundSymbols + (uint32_t)(tid >> 2) * kSegSymbols < n)
      seg_bit[r * (kBlockSymbols / kSegSymbols) + (uint32_t)(tid >> 2)] = seg_end;
    if (chunk_bit && tid == 0) chunk_bit[r] = B;
    const bool last = r + 1 == nrounds;
    uint32_t T = carry + round_bits;  // bits in the stage
    if (last) {  // the end mark, then 1-bits up to the byte (Buffer::flush_bits)
      const uint32_t pad = (0u - (T + end_len)) & 7u;
      if (tid == 0) {
        stage_put(S.stage, T, end_len, end_cw);
        if (pad) stage_put(S.stage, T + end_len, pad, (1u << pad) - 1u);
      }
      T += end_len + pad;
    }
    __syncthreads();  // the round's bits are complete
    const uint32_t base_byte = (B - carry) >> 3;
    const uint32_t full_units = T >> 7;
    const uint32_t units = last ? (T + 127u) >> 7 : full_units;
    for (uint32_t u = tid; u < units; u += kBatchThreads) {
      const uint4 q = *reinterpret_cast<const uint4*>(&S.stage[4 * u]);
      const uint32_t at = base_byte + 16u * u;
      if ((uint64_t)at + 16u <= image_bytes) {
        *reinterpret_cast<uint4*>(out + at) = make_uint4(bswap32(q.x), bswap32(q.y), bswap32(q.z), bswap32(q.w));
      } else {  // the image's last, incomplete unit: nothing behind the image is written
#pragma unroll
        for (uint32_t j = 0; j < 16; ++j) {
          const uint32_t w = j < 4 ? q.x : j < 8 ? q.y : j < 12 ? q.z : q.w;
          if ((uint64_t)at + j < image_bytes) out[at + j] = (uint8_t)(w >> (24 - 8 * (j & 3)));
        }
      }
    }
    const uint32_t keep = tid < 4 ? S.stage[4 * full_units + tid] : 0u;  // the bits of the incomplete unit go on
    __syncthreads();
    if (!last) {
      for (int w = tid; w < kBatchStageWords; w += kBatchThreads) S.stage[w] = 0;
      if (tid < 4) S.stage[tid] = keep;  // (this lane zeroed the word itself)
    }
    B += round_bits;
  }
  if (tid == 0) {
    P.out_bytes[item] = image_bytes;
    P.item_status[item] = GHF_OK;
  }
}

// ----------------------------------------------------------------------------------------------------------------------
// decode: the item's tables are checked and turned into a length-indexed direct table in LDS, lanes take 64-symbol
// segments from the item's side-car slice, the symbols of a round (256 segments) are staged in LDS and leave in 16-byte
// vectors wherever the output's alignment allows.  Every stream read is bounded by the item's stream_bytes: behind it
// the decoder reads zeros, whatever the side-car says.
// ----------------------------------------------------------------------------------------------------------------------
constexpr int kBatchDecRoundSegs = kBatchThreads;
constexpr int kBatchDecRoundBytes = kBatchDecRoundSegs * kSegSymbols;  // 16 KiB

struct BatchDecodeLds {
  uint16_t lut[1 << kDecLutBitsMax];  // sym | len << 9; 0: the code is longer than lut_bits
  uint32_t fcl[36];                   // first_code[len] << (32 - len); 0xFFFFFFFF outside [min_len, max_len]
  uint32_t sp[36];
  uint16_t symbol[GHF_NSYM + 3];
  alignas(16) uint32_t stage[kBatchDecRoundBytes / 4 + 4];
  unsigned long long kraft;
  int bad;
  int err;
};
static_assert(sizeof(BatchDecodeLds) <= 40 * 1024, "four workgroups per CU");

// big-endian word `wi` of the stream; zeros behind stream[0 .. bytes)
__device__ __forceinline__ uint32_t batch_stream_word(const uint8_t* __restrict__ s, uint64_t bytes, uint32_t wi) {
  const uint64_t b = 4ull * wi;
  if (b + 4 <= bytes) return bswap32(*reinterpret_cast<const uint32_t*>(s + b));
  uint32_t r = 0;
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j)
    if (b + j < bytes) r |= (uint32_t)s[b + j] << (24 - 8 * j);
  return r;
}

__global__ __launch_bounds__(kBatchThreads) void k_decode_batch(BatchDecodeParams P) {
  __shared__ BatchDecodeLds S;
  const int tid = threadIdx.x;
  const uint32_t item = blockIdx.x;
  const uint64_t n64 = P.n_symbols[item];
  const uint64_t stream_bytes = P.stream_bytes[item];
  const uint8_t* __restrict__ const stream = P.stream_ptrs[item];
  uint8_t* __restrict__ const out = P.out_ptrs[item];
  const ghf_code* __restrict__ const code = P.codes + item;
  int refuse = GHF_OK;
  if (n64 == 0) refuse = GHF_E_EMPTY;
  else if (n64 > P.max_item_bytes || !stream || !out || (reinterpret_cast<uintptr_t>(stream) & 15u)) refuse = GHF_E_INVAL;
  else if (n64 > P.out_caps[item]) refuse = GHF_E_CAP;
  const int max_len = code->max_len, min_len = code->min_len;
  if (!refuse && (max_len < 1 || max_len > 32 || min_len < 1 || min_len > max_len)) refuse = GHF_E_FORMAT;
  if (refuse) {
    if (tid == 0) {
      P.item_status[item] = refuse;
      P.out_bytes[item] = 0;
    }
    return;
  }
  const uint32_t n = (uint32_t)n64;
  // the checks of k_build_decode_tables: a complete prefix code (Kraft equality), lengths within [min_len, max_len],
  // first codes that fit their length, start positions inside symbol[]
  if (tid == 0) {
    S.kraft = 0;
    S.bad = 0;
    S.err = 0;
  }
  __syncthreads();
  {
    unsigned long long k = 0;
    int b = 0;
    for (int i = tid; i < GHF_NSYM; i += kBatchThreads) {
      const uint32_t l = code->length[i];
      if (l) {
        if ((int)l < min_len || (int)l > max_len) b = 1;
        else k += 1ull << (32 - l);
      }
    }
    uint32_t f = 0xFFFFFFFFu, p = 0;
    if (tid >= min_len && tid <= max_len) {
      const uint32_t fc = code->first_code[tid];
      p = code->start_pos[tid];
      if ((tid < 32 && fc > (1u << tid)) || p > (uint32_t)GHF_NSYM) b = 1;
      f = fc << (32 - tid);
    }
    if (tid < 36) {
      S.fcl[tid] = f;
      S.sp[tid] = p;
    }
    for (int i = tid; i < GHF_NSYM; i += kBatchThreads) S.symbol[i] = (uint16_t)(code->symbol[i] > 256u ? 256u : code->symbol[i]);
    if (k) atomicAdd(&S.kraft, k);
    if (b) atomicOr(&S.bad, 1);
  }
  __syncthreads();
  if (S.bad || S.kraft != (1ull << 32)) {
    if (tid == 0) {
      P.item_status[item] = GHF_E_FORMAT;
      P.out_bytes[item] = 0;
    }
    return;
  }
  const int lb = max_len < kDecLutBitsMax ? max_len : kDecLutBitsMax;
  for (uint32_t idx = tid; idx < (1u << lb); idx += kBatchThreads) {
    const uint32_t v = idx << (32 - lb);
    uint32_t ent = 0;
    for (int len = min_len; len <= lb; ++len) {
      if (v >= S.fcl[len]) {
        const uint32_t k = S.sp[len] + ((v - S.fcl[len]) >> (32 - len));
        ent = (k < (uint32_t)GHF_NSYM ? (uint32_t)S.symbol[k] : 256u) | ((uint32_t)len << 9);
        break;
      }
    }
    S.lut[idx] = (uint16_t)ent;
  }
  __syncthreads();

  const uint64_t* const chunk_bit = P.chunk_bit + (uint64_t)item * P.blocks_per_item;
  const uint32_t* const seg_bit = P.seg_bit + (uint64_t)item * P.segs_per_item;
  const uint64_t end_bit = stream_bytes * 8;
  const uint32_t nsegs = (n + kSegSymbols - 1) / kSegSymbols;
  const int long_from = lb + 1 > min_len ? lb + 1 : min_len;

#pragma unroll 1
  for (uint32_t s0 = 0; s0 < nsegs; s0 += kBatchDecRoundSegs) {
    const uint32_t s = s0 + (uint32_t)tid;
    if (s < nsegs) {
      const uint64_t B0 = chunk_bit[s >> 6];
      const uint32_t start = (s & 63u) ? seg_bit[s - 1] : 0u;
      const uint32_t end = seg_bit[s];
      const uint32_t cnt = n - s * kSegSymbols < (uint32_t)kSegSymbols ? n - s * kSegSymbols : (uint32_t)kSegSymbols;
      const bool is_last = s + 1 == nsegs;
      // bounds first: the segment (and the end mark behind the last one) lies inside the stream
      bool bad = end < start || B0 > end_bit || (uint64_t)end > end_bit - B0 || B0 + start > 0xFFFFFFFFull - 64u;
      uint32_t used = 0;
      if (!bad) {
        const uint32_t bit = (uint32_t)B0 + start;
        uint32_t wi = bit >> 5, o = bit & 31u;
        uint32_t hi = batch_stream_word(stream, stream_bytes, wi), lo = batch_stream_word(stream, stream_bytes, wi + 1);
        uint32_t word = 0;
        const uint32_t steps = cnt + (is_last ? 1u : 0u);
#pragma unroll 1
        for (uint32_t i = 0; i < steps; ++i) {
          const uint32_t win = (uint32_t)((((unsigned long long)hi << 32 | lo) << o) >> 32);
          uint32_t ent = S.lut[win >> (32 - lb)];
          if (ent == 0) {
            for (int len = long_from; len <= max_len; ++len) {
              const uint32_t f = S.fcl[len];
              if (win >= f) {
                const uint32_t k = S.sp[len] + ((win - f) >> (32 - len));
                ent = (k < (uint32_t)GHF_NSYM ? (uint32_t)S.symbol[k] : 256u) | ((uint32_t)len << 9);
                break;
              }
            }
          }
          const uint32_t sym = ent & 0x1FFu, len = ent >> 9;
          if (len == 0) {  // no code starts with these bits
            bad = true;
            break;
          }
          if (i < cnt) {
            if (sym == 256u) bad = true;  // an end mark among the data
            used += len;
            word |= (sym & 0xFFu) << (8 * (i & 3u));
            if ((i & 3u) == 3u || i + 1 == cnt) {
              S.stage[tid * 16 + (i >> 2)] = word;
              word = 0;
            }
          } else if (sym != 256u || (uint64_t)bit + used + len > end_bit) {
            bad = true;  // the end mark is missing behind the last symbol, or the stream ends inside it
          }
          o += len;
          if (o >= 32u) {
            o -= 32u;
            ++wi;
            hi = lo;
            lo = batch_stream_word(stream, stream_bytes, wi + 1);
          }
        }
        if (used != end - start) bad = true;  // the segment does not land on its recorded end
      }
      if (bad) S.err = 1;
    }
    __syncthreads();
    // the round's bytes leave: byte stores up to the first 16-byte boundary of out, vectors, byte stores at the end
    const uint32_t rb = s0 * kSegSymbols;
    const uint32_t rbytes = n - rb < (uint32_t)kBatchDecRoundBytes ? n - rb : (uint32_t)kBatchDecRoundBytes;
    uint8_t* const dst = out + rb;
    uint32_t head = (16u - ((uint32_t)reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u;
    head = head < rbytes ? head : rbytes;
    const uint8_t* const sb = reinterpret_cast<const uint8_t*>(S.stage);
    if ((uint32_t)tid < head) dst[tid] = sb[tid];
    const uint32_t nvec = (rbytes - head) >> 4;
    const uint32_t sh = 8u * (head & 3u);
    for (uint32_t q = tid; q < nvec; q += kBatchThreads) {
      const uint32_t at = head + 16u * q;
      const uint32_t* w = &S.stage[at >> 2];
      const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];
      *reinterpret_cast<uint4*>(dst + at) = make_uint4(alignbit(w1, w0, sh), alignbit(w2, w1, sh), alignbit(w3, w2, sh), alignbit(w4, w3, sh));
    }
    const uint32_t tail0 = head + 16u * nvec;
    if (tail0 + (uint32_t)tid < rbytes) dst[tail0 + tid] = sb[tail0 + tid];
    __syncthreads();
  }
  if (tid == 0) {
    const bool ok = S.err == 0;
    P.item_status[item] = ok ? GHF_OK : GHF_E_CORRUPT;
    P.out_bytes[item] = ok ? n : 0;
  }
}

void launch_compress_batch(const BatchCompressParams& p, uint32_t count, hipStream_t s) {
  if (count == 0) return;
  hipLaunchKernelGGL(k_compress_batch, dim3(count), dim3(kBatchThreads), 0, s, p);
}
void launch_decode_batch(const BatchDecodeParams& p, uint32_t count, hipStream_t s) {
  if (count == 0) return;
  hipLaunchKernelGGL(k_decode_batch, dim3(count), dim3(kBatchThreads), 0, s, p);
}

}  // namespace ghf
