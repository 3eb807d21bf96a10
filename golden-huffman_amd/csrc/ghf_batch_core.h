// golden-huffman_amd/csrc/ghf_batch_core.h -- the device helpers of the one-workgroup-per-item kernels, shared by
// ghf_batch.hip (one code per item), ghf_batch_shared.hip (one code for the batch), ghf_batch_planes.hip (one code per
// byte plane of the batch) and ghf_batch_seek.hip (stored bodies with a run record each): the round geometry, the item
// loads for any alignment, the LDS stage of the packer, the bounded stream reads and the bit cursor of the decoders, the
// packer of the shared-code kernels (batch_shared_compress_body, over a flat item or one byte plane of it), and what a
// decoder is made of: the table fill of one vetted code (batch_code_tables) with the code check in front of it
// (batch_code_ok), and the three round loops -- the one that follows a side-car (batch_decode_segments), the one that
// finds the code boundaries itself (batch_decode_rounds) and the one that follows a run record (batch_decode_runs) --
// each over the way its stage leaves (StoreFlat, StorePlane) -- and the raw form of a byte plane, packed and copied
// back without a code (batch_raw_compress_body, batch_raw_plane_copy).  Which kernels call them and which still carry a
// written-out copy, and why: profiles/batch_core/README.md; why the plane decoders and their raw-plane twins are still
// written out beside each other: profiles/batch_planes_bodies/README.md.
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
// bytes mis .. mis + 15 (mis = 1 .. 15) of the 32 bytes of two consecutive vectors, as four little-endian words
__device__ __forceinline__ uint4 batch_shift16(const uint4& a, const uint4& b, uint32_t mis) {
  uint32_t w0 = a.x, w1 = a.y, w2 = a.z, w3 = a.w, w4 = b.x, w5 = b.y, w6 = b.z, w7 = b.w;
  if (mis & 4u) { w0 = w1; w1 = w2; w2 = w3; w3 = w4; w4 = w5; w5 = w6; w6 = w7; }
  if (mis & 8u) { w0 = w2; w1 = w3; w2 = w4; w3 = w5; w4 = w6; }
  const uint32_t sh = 8u * (mis & 3u);
  return make_uint4(alignbit(w1, w0, sh), alignbit(w2, w1, sh), alignbit(w3, w2, sh), alignbit(w4, w3, sh));
}
// in[off .. off + 16) as four little-endian words, for any alignment of `in` (off is a multiple of 16, off < n).  Whole
// vectors come from one aligned 16-byte load, or from the two aligned vectors that hold them (the bytes in front of
// in[0] that this touches share a 16-byte granule with in[0]); the item's ragged end is read byte by byte.
__device__ __forceinline__ uint4 batch_load16(const uint8_t* __restrict__ in, uint32_t off, uint32_t n, uint32_t mis) {
  const uint8_t* p = in + off;
  if (off + 16u <= n) {
    if (mis == 0) return *reinterpret_cast<const uint4*>(p);
    return batch_shift16(*reinterpret_cast<const uint4*>(p - mis), *reinterpret_cast<const uint4*>(p - mis + 16), mis);
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

// ---- what one workgroup of the shared-code packer compresses (batch_shared_compress_body below) --------------------------
// open(): GHF_OK and n > 0 symbols, or what the item is refused with; load16(off): symbols off .. off + 15 as four
// little-endian words (off is a multiple of 16, off < n; zeros behind symbol n - 1).
struct FlatItem {  // the item's bytes as they lie
  const uint8_t* const* in_ptrs;
  const uint64_t* in_bytes;
  uint64_t max_item_bytes;
  uint32_t item;
  const uint8_t* __restrict__ in;
  uint32_t n, mis;
  __device__ __forceinline__ int open() {
    const uint64_t n64 = in_bytes[item];
    in = in_ptrs[item];
    if (n64 == 0) return GHF_E_EMPTY;
    if (n64 > max_item_bytes || !in) return GHF_E_INVAL;
    n = (uint32_t)n64;
    mis = (uint32_t)reinterpret_cast<uintptr_t>(in) & 15u;
    return GHF_OK;
  }
  __device__ __forceinline__ uint4 load16(uint32_t off) const { return batch_load16(in, off, n, mis); }
};

__device__ __forceinline__ uint32_t byte_perm(uint32_t hi, uint32_t lo, uint32_t sel) { return __builtin_amdgcn_perm(hi, lo, sel); }

// Byte plane p of an item of elements of E bytes: symbol k is in[k * E + p].  A lane's 16 symbols are the E consecutive
// 16-byte vectors at element offset off, loaded for any alignment by batch_load16's rule and narrowed to one vector in
// registers with the v_perm_b32 selections of ghf_planes.hip (p is the workgroup's: the selector is a scalar).  No LDS
// trip as in k_planes_split: the lane owns the whole row.  The ragged end is read byte by byte, nothing outside the item.
template <int E>
struct PlaneItem {
  static_assert(E == 2 || E == 4 || E == 8, "elements of 2, 4 or 8 bytes");
  const uint8_t* const* in_ptrs;
  const uint64_t* in_bytes;
  uint64_t max_item_bytes;
  uint32_t slot;  // item * E + p
  const uint8_t* __restrict__ al;  // the item's bytes are al[mis ..), al is 16-byte aligned
  uint32_t n, mis;                 // n symbols: n * E bytes
  __device__ __forceinline__ int open() {
    const uint32_t item = slot / E;
    const uint64_t n64 = in_bytes[item];
    const uint8_t* const in = in_ptrs[item];
    if (n64 == 0) return GHF_E_EMPTY;
    if (n64 > max_item_bytes || !in || n64 % E) return GHF_E_INVAL;  // (on all E slots of the item)
    n = (uint32_t)n64 / E;
    mis = (uint32_t)reinterpret_cast<uintptr_t>(in) & 15u;
    al = in - mis;
    return GHF_OK;
  }
  // G consecutive whole vectors of the item from byte b on (a multiple of 16): batch_load16's two cases, with the one
  // branch on the alignment around all the loads, so that they are in flight together; G + 1 aligned vectors hold G
  // unaligned ones (the last of them shares its first granule with the item's bytes)
  template <int G>
  __device__ __forceinline__ void vecs(uint32_t b, uint4 (&r)[G]) const {
    const uint4* const src = reinterpret_cast<const uint4*>(al + b);
    if (mis == 0) {
#pragma unroll
      for (int q = 0; q < G; ++q) r[q] = src[q];
    } else {
      uint4 t[G + 1];
#pragma unroll
      for (int q = 0; q <= G; ++q) t[q] = src[q];
#pragma unroll
      for (int q = 0; q < G; ++q) r[q] = batch_shift16(t[q], t[q + 1], mis);
    }
  }
  __device__ __forceinline__ uint4 load16(uint32_t off) const {
    const uint32_t b = off * E, p = slot % E;
    if (off + 16u <= n) {  // E whole vectors
      if constexpr (E == 2) {  // {a.b0 a.b2 b.b0 b.b2} or {a.b1 a.b3 b.b1 b.b3}
        const uint32_t sel = 0x06040200u + p * 0x01010101u;
        uint4 r[2];
        vecs(b, r);
        return make_uint4(byte_perm(r[0].y, r[0].x, sel), byte_perm(r[0].w, r[0].z, sel), byte_perm(r[1].y, r[1].x, sel),
                          byte_perm(r[1].w, r[1].z, sel));
      } else {  // byte p of four dwords; at E = 8 an element is a dword pair, narrowed first to a dword of its byte p
        const uint32_t sel = 0x04000400u + (E == 4 ? p : 0u) * 0x01010101u;  // {lo.bp hi.bp lo.bp hi.bp}
        auto four = [&](uint32_t e0, uint32_t e1, uint32_t e2, uint32_t e3) {
          return byte_perm(byte_perm(e3, e2, sel), byte_perm(e1, e0, sel), 0x05040100u);
        };
        uint32_t o[4];
        if constexpr (E == 4) {
          uint4 r[4];
          vecs(b, r);
#pragma unroll
          for (int q = 0; q < 4; ++q) o[q] = four(r[q].x, r[q].y, r[q].z, r[q].w);  // elements 4 q .. 4 q + 3 -> dword q
        } else {
          const uint32_t pick = p * 0x01010101u;
          auto two = [&](const uint4& v, uint32_t& e0, uint32_t& e1) { e0 = byte_perm(v.y, v.x, pick), e1 = byte_perm(v.w, v.z, pick); };
#pragma unroll
          for (int q = 0; q < 4; ++q) {  // elements 4 q .. 4 q + 3 -> dword q
            uint4 r[2];
            vecs(b + 32u * q, r);
            uint32_t e[4];
            two(r[0], e[0], e[1]);
            two(r[1], e[2], e[3]);
            o[q] = four(e[0], e[1], e[2], e[3]);
          }
        }
        return make_uint4(o[0], o[1], o[2], o[3]);
      }
    }
    uint32_t q0 = 0, q1 = 0, q2 = 0, q3 = 0;
#pragma unroll
    for (uint32_t j = 0; j < 16; ++j) {
      if (off + j < n) {
        const uint32_t v = (uint32_t)al[mis + b + j * E + p] << (8 * (j & 3));
        if (j < 4) q0 |= v;
        else if (j < 8) q1 |= v;
        else if (j < 12) q2 |= v;
        else q3 |= v;
      }
    }
    return make_uint4(q0, q1, q2, q3);
  }
};

// `len` bits (1..32) of `cw` at stage bit `pos`
__device__ __forceinline__ void stage_put(uint32_t* stage, uint32_t pos, uint32_t len, uint32_t cw) {
  const uint32_t w = pos >> 5, o = pos & 31u;
  const unsigned long long v = (unsigned long long)cw << (64u - o - len);
  atomicOr(&stage[w], (uint32_t)(v >> 32));
  if (o + len > 32u) atomicOr(&stage[w + 1], (uint32_t)v);
}

// ----------------------------------------------------------------------------------------------------------------------
// the packer of the shared-code kernels (k_compress_batch_shared: Item = FlatItem; k_compress_batch_planes_shared:
// PlaneItem<E>), one workgroup per output slot.  The code is checked once per workgroup (the rules k_decode_batch applies
// to an item's tables), a pricing pass gives the body's exact size before the first store, then the round loop of
// k_compress_batch packs from bit 0: no header words, no heap, no bins.
// ----------------------------------------------------------------------------------------------------------------------
struct BatchSharedCompressLds {
  uint2 tab[GHF_NSYM + 3];                       // (length, codeword)
  alignas(16) uint32_t stage[kBatchStageWords];  // the round's bits, MSB first
  uint32_t wave_bits[kBatchWaves];
  unsigned long long kraft;
  uint32_t body_bits;  // an item has at most 2^20 codes of <= 32 bits
  int bad;
  int nocode;
};
static_assert(sizeof(BatchSharedCompressLds) <= 20 * 1024, "eight workgroups per CU");

struct BatchSharedSlot {  // where one workgroup's body, size, status and side-car slice go
  const ghf_code* code;
  uint8_t* const* out_ptrs;  // [slot]
  const uint64_t* out_caps;
  uint64_t* out_bytes;
  int* item_status;
  uint64_t* chunk_bit;  // the side-car arrays (may both be null), slot j at j * blocks_per_item / j * segs_per_item
  uint32_t* seg_bit;
  uint64_t blocks_per_item, segs_per_item;
  uint32_t slot;
};

template <class Item>
__device__ __forceinline__ void batch_shared_compress_body(BatchSharedCompressLds& S, const BatchSharedSlot& W, Item it) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t slot = W.slot;
  const ghf_code* __restrict__ const code = W.code;
  auto finish = [&](int status, uint64_t bytes) {  // every lane of the workgroup takes the same exit
    if (tid == 0) {
      W.item_status[slot] = status;
      W.out_bytes[slot] = bytes;
    }
  };

  // ---- 1. the code: a complete prefix code of lengths <= 32 (ghf_code_rules.h, section 2) with a code for the end mark.
  // Nothing below trusts a length before this has passed: a table with a length of 60 never reaches the packer.
  const int max_len = code->max_len, min_len = code->min_len;
  if (!len_bounds_ok(min_len, max_len)) return finish(GHF_E_FORMAT, 0);
  if (tid == 0) {
    S.kraft = 0;
    S.body_bits = 0;
    S.bad = 0;
    S.nocode = 0;
  }
  __syncthreads();
  {
    unsigned long long k = 0;
    if (!code_share_ok(code, min_len, max_len, tid, kBatchThreads, &k)) atomicOr(&S.bad, 1);
    if (k) atomicAdd(&S.kraft, k);
    for (int s = tid; s < GHF_NSYM; s += kBatchThreads) {
      const uint32_t l = code->length[s];  // a codeword's bits above its length would land in its neighbours' bits
      S.tab[s] = make_uint2(l, code->codeword[s] & (l >= 32u ? 0xFFFFFFFFu : (1u << l) - 1u));
    }
    for (int w = tid; w < kBatchStageWords; w += kBatchThreads) S.stage[w] = 0;
  }
  __syncthreads();
  const uint32_t end_len = S.tab[GHF_NSYM - 1].x, end_cw = S.tab[GHF_NSYM - 1].y;
  if (S.bad || S.kraft != (1ull << 32) || end_len == 0) return finish(GHF_E_FORMAT, 0);

  const int refused = it.open();
  if (refused) return finish(refused, 0);
  uint8_t* __restrict__ const out = W.out_ptrs[slot];
  if (!out || (reinterpret_cast<uintptr_t>(out) & 15u)) return finish(GHF_E_INVAL, 0);
  const uint32_t n = it.n;

  // ---- 2. the price: the sum of the lengths, and whether a byte value without a code occurs ----
  {
    uint32_t bits = 0;
    bool none = false;
    for (uint32_t off = (uint32_t)tid * 16u; off < n; off += kBatchRoundSymbols) {
      const uint4 v = it.load16(off);
      const uint32_t cnt = n - off < 16u ? n - off : 16u;
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        if ((uint32_t)k < cnt) {
          const uint32_t l = S.tab[batch_byte(v, k)].x;
          bits += l;
          none |= l == 0;
        }
      }
    }
    const uint32_t incl = wave_incl_scan_u32(bits);
    if (lane == 63 && incl) atomicAdd(&S.body_bits, incl);
    if (none) S.nocode = 1;
  }
  __syncthreads();
  if (S.nocode) return finish(GHF_E_NOCODE, 0);

  // ---- 3. the cap, before the first store ----
  const uint32_t body_bytes = (S.body_bits + end_len + 7u) >> 3;
  if (body_bytes > W.out_caps[slot]) return finish(GHF_E_CAP, 0);

  uint64_t* const chunk_bit = W.chunk_bit ? W.chunk_bit + (uint64_t)slot * W.blocks_per_item : nullptr;
  uint32_t* const seg_bit = W.seg_bit ? W.seg_bit + (uint64_t)slot * W.segs_per_item : nullptr;

  // ---- 4. the round loop of k_compress_batch from body bit 0: one side-car block per round ----
  uint32_t B = 0;  // body bit of the next code
  const uint32_t nrounds = (n + kBatchRoundSymbols - 1) / kBatchRoundSymbols;
#pragma unroll 1
  for (uint32_t r = 0; r < nrounds; ++r) {
    const uint32_t off = r * kBatchRoundSymbols + (uint32_t)tid * 16u;
    const uint32_t cnt = off < n ? (n - off < 16u ? n - off : 16u) : 0u;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (cnt) v = it.load16(off);
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
      if (at + 16u <= body_bytes) {
        *reinterpret_cast<uint4*>(out + at) = make_uint4(bswap32(q.x), bswap32(q.y), bswap32(q.z), bswap32(q.w));
      } else {  // the body's last, incomplete unit: nothing behind the body is written
#pragma unroll
        for (uint32_t j = 0; j < 16; ++j) {
          const uint32_t w = j < 4 ? q.x : j < 8 ? q.y : j < 12 ? q.z : q.w;
          if (at + j < body_bytes) out[at + j] = (uint8_t)(w >> (24 - 8 * (j & 3)));
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
  finish(GHF_OK, body_bytes);
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

// ---- the way out of the stage, a template parameter of the decoders' round loops: store(out, base, stage, rbytes, tid)
// puts stage[0 .. rbytes) behind the `base` symbols the rounds before it wrote
struct StoreFlat {  // out[base + s]: the item's bytes as they lie
  __device__ __forceinline__ void operator()(uint8_t* out, uint32_t base, const uint32_t* stage, uint32_t rbytes, int tid) const {
    batch_store_stage(out + base, stage, rbytes, tid);
  }
};
template <int E>
struct StorePlane {  // out[(base + s) * E + p]: byte plane p of elements of E bytes; one byte store per symbol at stride E
  uint32_t p;
  __device__ __forceinline__ void operator()(uint8_t* out, uint32_t base, const uint32_t* stage, uint32_t rbytes, int tid) const {
    const uint8_t* const sb = reinterpret_cast<const uint8_t*>(stage);
    uint8_t* const dst = out + (base * E + p);  // fits 32 bits: a body of <= 2^25 bits holds fewer than 2^25 symbols
    for (uint32_t s = tid; s < rbytes; s += kBatchThreads) dst[s * E] = sb[s];
  }
};

// ----------------------------------------------------------------------------------------------------------------------
// the round loop of the decoders that follow a live side-car (k_decode_batch_shared, k_decode_batch_planes_shared; written
// out once more in k_decode_batch): rounds of 256 segments of 64 symbols, one per lane, from the recorded bit of each.  Every
// lane of the workgroup calls it with the same arguments; S.t holds the filled tables (a barrier lies behind
// batch_code_tables).  Every segment must land on its recorded end and the end mark must follow the last symbol: S.err
// (zero when the first call starts) is raised otherwise, and the round is stored all the same.  No byte outside stream[0 .. stream_bytes) is read.  (No __restrict__
// on stream / out: with it the compiler unrolls batch_store_stage's vector loop with dword stores.)
// ----------------------------------------------------------------------------------------------------------------------
template <class Lds, class Store>  // Lds: the kernel's __shared__ struct with a CodeTab t, the stage and an int err
__device__ __forceinline__ void batch_decode_segments(Lds& S, const uint8_t* stream, uint64_t stream_bytes,
                                                      const uint64_t* chunk_bit, const uint32_t* seg_bit, uint32_t n, uint8_t* out,
                                                      int lb, int long_from, int max_len, const Store& store) {
  const int tid = threadIdx.x;
  const uint64_t end_bit = stream_bytes * 8;
  const uint32_t nsegs = (uint32_t)segs_for(n);
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
        BatchCursor cur;
        cur.seek(stream, stream_bytes, bit);
        uint32_t word = 0;
        const uint32_t steps = cnt + (is_last ? 1u : 0u);
#pragma unroll 1
        for (uint32_t i = 0; i < steps; ++i) {
          const uint32_t ent = batch_decode_one(S.t, cur.window(), lb, long_from, max_len);
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
          cur.skip(stream, stream_bytes, len);
        }
        if (used != end - start) bad = true;  // the segment does not land on its recorded end
      }
      if (bad) S.err = 1;
    }
    __syncthreads();
    // the round's bytes leave
    const uint32_t rb = s0 * kSegSymbols;
    const uint32_t rbytes = n - rb < (uint32_t)kBatchDecRoundBytes ? n - rb : (uint32_t)kBatchDecRoundBytes;
    store(out, rb, S.stage, rbytes, tid);
    __syncthreads();
  }
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
// is read; under kWrite only out[0 .. min(total, cap)) is written (through `store`: those symbols' places).  rounds /
// passes: += what the item took.  R is as batch_rounds_init left it.
template <bool kWrite, class Store = StoreFlat>
__device__ __forceinline__ int batch_decode_rounds(const CodeTab& T, uint32_t* stage, BatchRoundsLds& R,
                                                   const uint8_t* __restrict__ stream, uint64_t stream_bytes, uint32_t first_bit,
                                                   uint64_t cap, uint8_t* __restrict__ out, int lb, int long_from, int max_len,
                                                   uint32_t* total_out, uint32_t& rounds, uint32_t& passes,
                                                   const Store& store = Store()) {
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
        store(out, total + lo, stage, rbytes, tid);
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

// ----------------------------------------------------------------------------------------------------------------------
// the front of the decoders that are handed a ghf_code, stated once: the code check (ghf_batch_seek.hip) and the table
// fill (ghf_batch_seek.hip, ghf_batch_planes.hip, whose E codes are vetted in one go by planes_codes_ok).  k_decode_batch,
// k_decode_batch_shared and k_decode_bodies_batch_shared keep their written-out copies of both: called from there the
// functions re-lay those kernels, and the measurement that has to clear a re-laid listing was not made
// (profiles/batch_core/README.md; DESIGN.md sections 11, 13 and 16).
// ----------------------------------------------------------------------------------------------------------------------
struct CodeVetLds {
  unsigned long long kraft;
  int bad;
};
// every lane of the workgroup; barriers on both sides are inside.  -> `code` is a complete prefix code of lengths <= 32
// (ghf_code_rules.h, section 2)
__device__ __forceinline__ bool batch_code_ok(CodeVetLds& V, const ghf_code* __restrict__ code, int tid) {
  const int max_len = code->max_len, min_len = code->min_len;
  __syncthreads();  // the lanes are done with what the call before this one left in V
  if (tid == 0) {
    V.kraft = 0;
    V.bad = len_bounds_ok(min_len, max_len) ? 0 : 1;
  }
  __syncthreads();
  if (len_bounds_ok(min_len, max_len)) {  // (the same in every lane) nothing below trusts a length before this has passed
    unsigned long long k = 0;
    if (!code_share_ok(code, min_len, max_len, tid, kBatchThreads, &k)) atomicOr(&V.bad, 1);
    if (k) atomicAdd(&V.kraft, k);
  }
  __syncthreads();
  return V.bad == 0 && V.kraft == (1ull << 32);
}
// the tables of one vetted code; every lane of the workgroup, barriers on both sides are inside
__device__ __forceinline__ void batch_code_tables(CodeTab& T, const ghf_code* __restrict__ code, int tid, int& lb, int& long_from,
                                                  int& max_len) {
  const int min_len = code->min_len;
  max_len = code->max_len;
  __syncthreads();  // the lanes are done with the tables of the code before this one
  if (tid < 36) tab_load_row(T, tid, min_len, max_len, code->first_code, code->start_pos);
  for (int i = tid; i < GHF_NSYM; i += kBatchThreads) T.symbol[i] = tab_symbol(code->symbol[i]);
  __syncthreads();
  lb = max_len < kDecLutBitsMax ? max_len : kDecLutBitsMax;
  long_from = lb + 1 > min_len ? lb + 1 : min_len;
  tab_fill_lut(T, min_len, lb, tid, kBatchThreads);
  __syncthreads();
}

// ----------------------------------------------------------------------------------------------------------------------
// the round loop of the decoders that follow a stored run record (k_decode_bodies_batch_shared_seek and its planes form):
// rounds of 256 runs of 128 symbols, one per lane.  Lane t loads run_bits[r0 + t]; a workgroup scan plus the bits of the
// rounds before gives the bit its run starts at; the lane decodes its run once, straight into the stage, and must land
// on the recorded end (behind the last run the end mark must follow, whole).  Every lane of the workgroup calls it with
// the same arguments; S.t holds the filled tables (a barrier lies behind batch_code_tables).  S.err (zero when the first
// call starts) is raised on the first round that fails, and that round and the ones behind it are not stored.  Nothing in
// the record is trusted: run_bits[] is [0, ceil(n / 128)) u16 behind the record's 8 header bytes, which the caller has
// held against the record's size; no byte outside stream[0 .. stream_bytes) is read (stream_bytes * 8 fits 32 bits, and
// so does any sum of 8192 run lengths).
//
// The stage is linear -- symbol s of the round at byte s -- so that StoreFlat / StorePlane take it as they take the
// stages above.  A lane's run is 128 consecutive bytes, so lanes lie 32 banks apart and a dword store per four symbols
// would put the 64 lanes of a wave on two banks; the lane collects 16 symbols in four registers and writes them with one
// ds_write_b128 instead: an eighth of the stores, each touching four banks.
// ----------------------------------------------------------------------------------------------------------------------
constexpr uint32_t kBatchSeekRoundRuns = kBatchThreads;
constexpr uint32_t kBatchSeekRoundBytes = kBatchSeekRoundRuns * kBatchRunSymbols;  // 32 KiB

template <class Lds, class Store>  // Lds: a CodeTab t, stage[kBatchSeekRoundBytes / 4 + 4], wave_bits[kBatchWaves], an int err
__device__ __forceinline__ void batch_decode_runs(Lds& S, const uint8_t* stream, uint64_t stream_bytes, const uint8_t* rec, uint32_t n,
                                                  uint8_t* out, int lb, int long_from, int max_len, const Store& store) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t end_bit = (uint32_t)stream_bytes * 8u;
  const uint32_t nruns = (uint32_t)batch_runs_for(n);
  const uint16_t* const run_bits = reinterpret_cast<const uint16_t*>(rec + kBatchSeekHeadBytes);
  uint32_t carry = 0;  // the bits of the rounds before this one
#pragma unroll 1
  for (uint32_t r0 = 0; r0 < nruns; r0 += kBatchSeekRoundRuns) {
    const uint32_t run = r0 + (uint32_t)tid;
    const uint32_t bits = run < nruns ? (uint32_t)run_bits[run] : 0u;
    const uint32_t incl = wave_incl_scan_u32(bits);
    if (lane == 63) S.wave_bits[wave] = incl;
    __syncthreads();
    uint32_t before = 0, round_bits = 0;
#pragma unroll
    for (int w = 0; w < kBatchWaves; ++w) {
      const uint32_t t = S.wave_bits[w];
      before += w < wave ? t : 0u;
      round_bits += t;
    }
    if (run < nruns) {
      const uint32_t start = carry + before + incl - bits;
      const uint32_t cnt = n - run * kBatchRunSymbols < kBatchRunSymbols ? n - run * kBatchRunSymbols : kBatchRunSymbols;
      const bool is_last = run + 1 == nruns;
      // bounds first: the run lies inside the stream (the end mark behind the last one is held as it is decoded)
      bool bad = start > end_bit || bits > end_bit - start;
      if (!bad) {
        BatchCursor cur;
        cur.seek(stream, stream_bytes, start);
        uint32_t used = 0;
        uint4 q = make_uint4(0, 0, 0, 0);  // the last four words of symbols, oldest first
        uint4* const mine = reinterpret_cast<uint4*>(&S.stage[tid * (kBatchRunSymbols / 4)]);
        const uint32_t nwords = (cnt + 3u) >> 2;
#pragma unroll 1
        for (uint32_t w = 0; w < nwords && !bad; ++w) {
          uint32_t word = 0;
#pragma unroll
          for (uint32_t k = 0; k < 4; ++k) {
            if (4u * w + k < cnt) {
              const uint32_t ent = batch_decode_one(S.t, cur.window(), lb, long_from, max_len);
              const uint32_t sym = ent & 0x1FFu, len = ent >> 9;
              if (len == 0 || sym == 256u) bad = true;  // no code starts with these bits, or an end mark among the data
              used += len;
              word |= (sym & 0xFFu) << (8u * k);
              cur.skip(stream, stream_bytes, len);
            }
          }
          q = make_uint4(q.y, q.z, q.w, word);
          if ((w & 3u) == 3u) mine[w >> 2] = q;
        }
        if (!bad && (nwords & 3u)) {  // the run's last, incomplete group of 16
#pragma unroll 1
          for (uint32_t w = nwords & 3u; w < 4u; ++w) q = make_uint4(q.y, q.z, q.w, 0u);
          mine[nwords >> 2] = q;
        }
        if (used != bits) bad = true;  // the run does not land on its recorded end
        if (!bad && is_last) {
          const uint32_t ent = batch_decode_one(S.t, cur.window(), lb, long_from, max_len);
          const uint32_t len = ent >> 9;
          // the end mark is missing behind the last symbol, or the stream ends inside it
          if (len == 0 || (ent & 0x1FFu) != 256u || len > end_bit - (start + bits)) bad = true;
        }
      }
      if (bad) S.err = 1;
    }
    __syncthreads();
    if (S.err) return;  // (the same in every lane)
    const uint32_t rb = r0 * kBatchRunSymbols;
    const uint32_t rbytes = n - rb < kBatchSeekRoundBytes ? n - rb : kBatchSeekRoundBytes;
    store(out, rb, S.stage, rbytes, tid);
    __syncthreads();
    carry += round_bits;
  }
}

// ----------------------------------------------------------------------------------------------------------------------
// the raw form of a byte plane of the batch: slot j = i * E + p holds the n bytes in[p], in[p + E],
// .. of item i and nothing else -- no code, no header, no end mark.  batch_raw_compress_body is what a workgroup of the
// forms packer runs for a raw slot in place of batch_shared_compress_body; batch_raw_plane_copy is what the forms
// decoders run for a raw plane in place of the table fill and the round loop.
// ----------------------------------------------------------------------------------------------------------------------
// the verdicts and their order are batch_shared_compress_body's without the code's: the item, the slot's pointer, the cap
// -- all before the first store.  Each lane takes rows of 16 symbols through PlaneItem::load16 (E vectors narrowed with
// v_perm_b32, at any alignment of the item) and stores one vector to the aligned slot; the ragged end goes byte by
// byte, nothing at or beyond n is written.  No pricing pass, no table, no LDS.
template <int E>
__device__ __forceinline__ void batch_raw_compress_body(const BatchSharedSlot& W, PlaneItem<E> it) {
  const int tid = threadIdx.x;
  const uint32_t slot = W.slot;
  auto finish = [&](int status, uint64_t bytes) {  // every lane of the workgroup takes the same exit
    if (tid == 0) {
      W.item_status[slot] = status;
      W.out_bytes[slot] = bytes;
    }
  };
  const int refused = it.open();
  if (refused) return finish(refused, 0);
  uint8_t* __restrict__ const out = W.out_ptrs[slot];
  if (!out || (reinterpret_cast<uintptr_t>(out) & 15u)) return finish(GHF_E_INVAL, 0);
  const uint32_t n = it.n;
  if (n > W.out_caps[slot]) return finish(GHF_E_CAP, 0);
  for (uint32_t off = (uint32_t)tid * 16u; off < n; off += kBatchRoundSymbols) {
    const uint4 v = it.load16(off);
    if (off + 16u <= n) {
      *reinterpret_cast<uint4*>(out + off) = v;
    } else {
#pragma unroll
      for (uint32_t j = 0; j < 16; ++j)
        if (off + j < n) out[off + j] = (uint8_t)batch_byte(v, (int)j);
    }
  }
  finish(GHF_OK, n);
}

// stream[0 .. n) -> out[k * E + p]: rounds of stage_bytes (a multiple of 16; the stage keeps four spare words behind them)
// -- 16-byte loads of the aligned slot into the stage, then the strided byte stores of StorePlane<E>, so that a wave's
// stores fall on consecutive elements as the dense planes' do.  The stream's ragged end is read byte by byte: no byte
// outside stream[0 .. n) is read.  Every lane of the workgroup calls it with the same arguments; nobody reads the stage
// when it starts (a barrier lies behind the plane before), and a barrier closes the last round.
template <int E>
__device__ __forceinline__ void batch_raw_plane_copy(uint32_t* stage, uint32_t stage_bytes, const uint8_t* stream, uint32_t n,
                                                     uint8_t* out, uint32_t p, int tid) {
#pragma unroll 1
  for (uint32_t rb = 0; rb < n; rb += stage_bytes) {
    const uint32_t rbytes = n - rb < stage_bytes ? n - rb : stage_bytes;
    for (uint32_t q = (uint32_t)tid * 16u; q < rbytes; q += kBatchThreads * 16u) {
      const uint32_t off = rb + q;
      uint4 v;
      if (off + 16u <= n) {
        v = *reinterpret_cast<const uint4*>(stream + off);
      } else {
        uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
        for (uint32_t j = 0; j < 16; ++j)
          if (off + j < n) w[j >> 2] |= (uint32_t)stream[off + j] << (8 * (j & 3));
        v = make_uint4(w[0], w[1], w[2], w[3]);
      }
      *reinterpret_cast<uint4*>(&stage[q >> 2]) = v;
    }
    __syncthreads();
    StorePlane<E>{p}(out, rb, stage, rbytes, tid);
    __syncthreads();
  }
}

// a raw slot's size as a symbol count: 1 .. GHF_BATCH_MAX_ITEM / E (the decoders that have nothing else to go by)
template <int E>
__device__ __forceinline__ bool batch_raw_count_ok(uint64_t stream_bytes) {
  return stream_bytes != 0 && stream_bytes <= GHF_BATCH_MAX_ITEM / E;
}

}  // namespace ghf
#endif
