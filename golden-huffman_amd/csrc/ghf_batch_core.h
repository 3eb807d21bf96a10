// golden-huffman_amd/csrc/ghf_batch_core.h -- the device helpers of the one-workgroup-per-item kernels, shared by
// ghf_batch.hip (one code per item) and ghf_batch_shared.hip (one code for the batch): the round geometry, the item
// loads for any alignment, the LDS stage of the packer, the bounded stream reads and the bit cursor of the decoders.
#ifndef GHF_BATCH_CORE_H_
#define GHF_BATCH_CORE_H_
#include "ghf_code_rules.h"
#include "ghf_device.h"

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

// `len` bits (1..32) of `cw` at stage bit `pos`
__device__ __forceinline__ void stage_put(uint32_t* stage, uint32_t pos, uint32_t len, uint32_t cw) {
  const uint32_t w = pos >> 5, o = pos & 31u;
  const unsigned long long v = (unsigned long long)cw << (64u - o - len);
  atomicOr(&stage[w], (uint32_t)(v >> 32));
  if (o + len > 32u) atomicOr(&stage[w + 1], (uint32_t)v);
}

constexpr int kBatchDecRoundSegs = kBatchThreads;
constexpr int kBatchDecRoundBytes = kBatchDecRoundSegs * kSegSymbols;  // 16 KiB

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

// sym | len << 9 of the code the 32-bit window starts with; len == 0: no code does
__device__ __forceinline__ uint32_t batch_decode_one(const CodeTab& T, uint32_t win, int lb, int long_from, int max_len) {
  const uint32_t ent = T.lut[win >> (32 - lb)];
  return ent ? ent : tab_search(T, win, long_from, max_len);
}

// the bit cursor of the batch decoders: 64 stream bits from word `wi` on, `o` (< 32) of them consumed
struct BatchCursor {
  uint32_t hi, lo, wi, o;
  __device__ __forceinline__ void seek(const uint8_t* __restrict__ s, uint64_t bytes, uint32_t bit) {
    wi = bit >> 5;
    o = bit & 31u;
    hi = batch_stream_word(s, bytes, wi);
    lo = batch_stream_word(s, bytes, wi + 1);
  }
  __device__ __forceinline__ uint32_t window() const { return (uint32_t)((((unsigned long long)hi << 32 | lo) << o) >> 32); }
  __device__ __forceinline__ void skip(const uint8_t* __restrict__ s, uint64_t bytes, uint32_t len) {
    o += len;
    if (o >= 32u) {
      o -= 32u;
      ++wi;
      hi = lo;
      lo = batch_stream_word(s, bytes, wi + 1);
    }
  }
};

// stage[0 .. rbytes) -> dst: byte stores up to the first 16-byte boundary of dst, vectors, byte stores at the end (the
// stage keeps four spare words behind its last byte)
__device__ __forceinline__ void batch_store_stage(uint8_t* dst, const uint32_t* stage, uint32_t rbytes, int tid) {
  uint32_t head = (16u - ((uint32_t)reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u;
  head = head < rbytes ? head : rbytes;
  const uint8_t* const sb = reinterpret_cast<const uint8_t*>(stage);
  if ((uint32_t)tid < head) dst[tid] = sb[tid];
  const uint32_t nvec = (rbytes - head) >> 4;
  const uint32_t sh = 8u * (head & 3u);
  for (uint32_t q = tid; q < nvec; q += kBatchThreads) {
    const uint32_t at = head + 16u * q;
    const uint32_t* w = &stage[at >> 2];
    const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];
    *reinterpret_cast<uint4*>(dst + at) = make_uint4(alignbit(w1, w0, sh), alignbit(w2, w1, sh), alignbit(w3, w2, sh), alignbit(w4, w3, sh));
  }
  const uint32_t tail0 = head + 16u * nvec;
  if (tail0 + (uint32_t)tid < rbytes) dst[tail0 + tid] = sb[tail0 + tid];
}

}  // namespace ghf
#endif
