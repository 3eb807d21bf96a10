// golden-huffman_amd/csrc/ghf_batch_core.h -- the device helpers of the one-workgroup-per-item kernels, shared by
// ghf_batch.hip (one code per item) and ghf_batch_shared.hip (one code for the batch): the round geometry, the item
// loads for any alignment, the LDS stage of the packer, the bounded stream reads and the bit cursor of the decoders, and
// the round loop of the decoders that find the code boundaries themselves (batch_decode_rounds).
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

// ----------------------------------------------------------------------------------------------------------------------
// the round loop of the decoders that get nothing but the bytes (k_decode_images_batch, DESIGN.md section 10;
// k_decode_bodies_batch_shared, section 13): the workgroup finds the code boundaries itself.  Rounds of 256 subsequences
// of 512 bits, one per lane, settled by passes in which lane k restarts from where lane k - 1 landed until nothing moves
// at or in front of the first end mark (lane 0 starts at an exactly known bit, so the fixed point is the true
// segmentation).  A scan of the lanes' symbol counts gives the output offsets; under kWrite the lanes decode once more
// into a 16 KiB stage that leaves slice by slice.
// ----------------------------------------------------------------------------------------------------------------------
constexpr uint32_t kImgSubBits = 512;
constexpr uint32_t kImgRoundBits = kBatchThreads * kImgSubBits;
constexpr uint32_t kImgStageBytes = 16 * 1024;
constexpr uint32_t kImgNone = 0xFFFFFFFFu;
constexpr uint32_t kImgEndMark = 1, kImgCutOff = 2;  // why a lane stopped inside its subsequence

struct BatchRoundsLds {  // next to a CodeTab and a stage of kImgStageBytes / 4 + 4 words
  uint16_t over[2][kBatchThreads];  // bits each lane's last code runs past its subsequence; written in pass p, read in p + 1
  uint32_t mins[3][2];              // [pass % 3]{first lane whose start moved, first lane that met the end (mark) of the stream}
  uint32_t wave_tot[kBatchWaves];
  uint32_t stop_kind;
};
// tid 0, with a barrier between this and batch_decode_rounds
__device__ __forceinline__ void batch_rounds_init(BatchRoundsLds& R) {
  for (int b = 0; b < 3; ++b) R.mins[b][0] = R.mins[b][1] = kImgNone;
}

// Every lane of the workgroup calls it with the same arguments; T holds the filled tables (a barrier lies behind
// tab_fill_lut).  The first code starts at stream bit `first_bit`; stream_bytes * 8 fits 32 bits.  -> GHF_OK and *total =
// the symbols in front of the first end mark, GHF_E_CORRUPT (the stream ends before a whole end mark) or GHF_E_CAP (more
// than `cap` symbols; seen before any store of the round that would cross it).  No byte outside stream[0 .. stream_bytes)
// is read; under kWrite only out[0 .. min(total, cap)) is written.  rounds / passes: += what the item took.
template <bool kWrite>
__device__ __forceinline__ int batch_decode_rounds(const CodeTab& T, uint32_t* stage, BatchRoundsLds& R,
                                                   const uint8_t* __restrict__ stream, uint64_t stream_bytes, uint32_t first_bit,
                                                   uint64_t cap, uint8_t* __restrict__ out, int lb, int long_from, int max_len,
                                                   uint32_t* total_out, uint32_t& rounds, uint32_t& passes) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t end_bit = (uint32_t)stream_bytes * 8u;
  uint32_t base = first_bit;  // first bit of the round's subsequence 0
  uint32_t carry = 0;         // bits the previous round's last code runs into this one: lane 0's start, exact
  uint32_t total = 0;         // symbols of the rounds before this one
  uint32_t pb = 0, po = 0;    // pass % 3, pass % 2
#pragma unroll 1
  for (;;) {
    ++rounds;
    const uint32_t sub0 = base + (uint32_t)tid * kImgSubBits, sub_end = sub0 + kImgSubBits;
    uint32_t start = kImgNone, cnt = 0, stop = 0, over = 0;
    uint32_t round_passes = 0, first_stop;
#pragma unroll 1
    for (;;) {
      const uint32_t in = tid == 0 ? carry : round_passes == 0 ? 0u : (uint32_t)R.over[po][tid - 1];
      const bool moved = in != start;
      if (moved) {  // code lengths only, from `in` until the lane leaves its subsequence, the end mark or the stream's end
        start = in;
        cnt = 0;
        stop = 0;
        uint32_t pos = sub0 + in;
        BatchCursor cur;
        cur.seek(stream, stream_bytes, pos);
#pragma unroll 1
        while (pos < sub_end) {
          const uint32_t ent = batch_decode_one(T, cur.window(), lb, long_from, max_len);
          const uint32_t len = ent >> 9;
          if (len == 0 || pos >= end_bit || len > end_bit - pos) {  // the code (an end mark too) must lie wholly inside the stream
            stop = kImgCutOff;
            break;
          }
          if ((ent & 0x1FFu) == 256u) {
            stop = kImgEndMark;
            break;
          }
          ++cnt;
          pos += len;
          cur.skip(stream, stream_bytes, len);
        }
        over = stop ? 0u : pos - sub_end;
      }
      R.over[po ^ 1u][tid] = (uint16_t)over;
      const unsigned long long m_moved = __ballot(moved), m_stop = __ballot(stop != 0);
      if (lane == 0) {
        if (m_moved) atomicMin(&R.mins[pb][0], (uint32_t)(wave * 64 + __builtin_ctzll(m_moved)));
        if (m_stop) atomicMin(&R.mins[pb][1], (uint32_t)(wave * 64 + __builtin_ctzll(m_stop)));
      }
      const uint32_t nb = pb == 2 ? 0u : pb + 1;
      if (tid == 0) R.mins[nb][0] = R.mins[nb][1] = kImgNone;  // last read two barriers ago, next written behind this one
      __syncthreads();
      const uint32_t first_moved = R.mins[pb][0];
      first_stop = R.mins[pb][1];
      pb = nb;
      po ^= 1u;
      ++round_passes;
      // settled: nothing moved at or in front of the first stop -- and lanes 0 .. p are exact after pass p in any case
      if (first_moved == kImgNone || first_moved > first_stop || first_stop < round_passes) break;
    }
    passes += round_passes;
    const uint32_t mine = (uint32_t)tid <= first_stop ? cnt : 0u;  // (first_stop == kImgNone: every lane counts)
    const uint32_t incl = wave_incl_scan_u32(mine);
    if (lane == 63) R.wave_tot[wave] = incl;
    if ((uint32_t)tid == first_stop) R.stop_kind = stop;
    __syncthreads();
    uint32_t before = 0, round_total = 0;
#pragma unroll
    for (int w = 0; w < kBatchWaves; ++w) {
      const uint32_t t = R.wave_tot[w];
      before += w < wave ? t : 0u;
      round_total += t;
    }
    const uint32_t stop_kind = first_stop == kImgNone ? 0u : R.stop_kind;
    if (stop_kind == kImgCutOff) return GHF_E_CORRUPT;  // the stream ends before a whole end mark
    if ((uint64_t)total + round_total > cap) return GHF_E_CAP;  // before any store of the round
    if (kWrite) {
      const uint32_t rel = before + incl - mine;  // of the lane's first symbol in the round's output
      uint32_t i = 0;
      BatchCursor cur;
      if (mine) cur.seek(stream, stream_bytes, sub0 + start);
      uint8_t* const sb = reinterpret_cast<uint8_t*>(stage);
#pragma unroll 1
      for (uint32_t lo = 0; lo < round_total; lo += kImgStageBytes) {  // (min_len 1: a round holds up to 128 Ki symbols)
        while (i < mine && rel + i < lo + kImgStageBytes) {
          const uint32_t ent = batch_decode_one(T, cur.window(), lb, long_from, max_len);
          sb[rel + i - lo] = (uint8_t)ent;
          cur.skip(stream, stream_bytes, ent >> 9);
          ++i;
        }
        __syncthreads();
        const uint32_t rbytes = round_total - lo < kImgStageBytes ? round_total - lo : kImgStageBytes;
        batch_store_stage(out + total + lo, stage, rbytes, tid);
        __syncthreads();
      }
    }
    total += round_total;
    if (stop_kind == kImgEndMark) {
      *total_out = total;
      return GHF_OK;
    }
    carry = R.over[po][kBatchThreads - 1];
    base += kImgRoundBits;
  }
}

}  // namespace ghf
#endif
