// golden-huffman_amd/csrc/ghf_batch.hip -- many small independent .crs2 streams in one launch per direction
// (ghf_compress_batch / ghf_decode_batch, include/ghf.h).
//
// One workgroup owns one item from its first byte to its last, so nothing crosses a workgroup: no workspace scans, no
// 16-byte unit with two writers, no atomics to memory and no pre-zeroed output.  What the single-stream path spreads
// over five launches (K1, K2+K3, K4, K5 and the header) happens inside the workgroup; the one-wavefront code build, which
// costs a looping caller 0.26 ms per item on an idle GPU, is hidden by the other workgroups resident on the same CU.
#include "ghf_batch_core.h"
#include "ghf_build_code.h"
#include "ghf_code_rules.h"

namespace ghf {

struct LdsCounts {  // the workgroup's 256 byte counts; the end mark counts once (include/encoder.h:123-129)
  static constexpr bool kAnyCount = false;  // 32-bit bins of an item of at most 1 MiB: far inside the builder's domain
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
  const uint32_t hdr_bytes = header_bytes_for((uint32_t)max_len);
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
struct BatchDecodeLds {
  CodeTab t;  // the item's decode tables (ghf_code_rules.h)
  alignas(16) uint32_t stage[kBatchDecRoundBytes / 4 + 4];
  unsigned long long kraft;
  int bad;
  int err;
};
static_assert(sizeof(BatchDecodeLds) <= 40 * 1024, "four workgroups per CU");

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
  if (!refuse && !len_bounds_ok(min_len, max_len)) refuse = GHF_E_FORMAT;
  if (refuse) {
    if (tid == 0) {
      P.item_status[item] = refuse;
      P.out_bytes[item] = 0;
    }
    return;
  }
  const uint32_t n = (uint32_t)n64;
  // a complete prefix code (ghf_code_rules.h, section 2), and its tables
  if (tid == 0) {
    S.kraft = 0;
    S.bad = 0;
    S.err = 0;
  }
  __syncthreads();
  {
    unsigned long long k = 0;
    if (!code_share_ok(code, min_len, max_len, tid, kBatchThreads, &k)) atomicOr(&S.bad, 1);
    if (k) atomicAdd(&S.kraft, k);
    if (tid < 36) tab_load_row(S.t, tid, min_len, max_len, code->first_code, code->start_pos);
    for (int i = tid; i < GHF_NSYM; i += kBatchThreads) S.t.symbol[i] = tab_symbol(code->symbol[i]);
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
  tab_fill_lut(S.t, min_len, lb, tid, kBatchThreads);
  __syncthreads();

  const uint64_t* const chunk_bit = P.chunk_bit + (uint64_t)item * P.blocks_per_item;
  const uint32_t* const seg_bit = P.seg_bit + (uint64_t)item * P.segs_per_item;
  const uint64_t end_bit = stream_bytes * 8;
  const uint32_t nsegs = (uint32_t)segs_for(n);
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
    batch_store_stage(out + rb, S.stage, rbytes, tid);
    __syncthreads();
  }
  if (tid == 0) {
    const bool ok = S.err == 0;
    P.item_status[item] = ok ? GHF_OK : GHF_E_CORRUPT;
    P.out_bytes[item] = ok ? n : 0;
  }
}

// ----------------------------------------------------------------------------------------------------------------------
// decode of standalone images (ghf_decode_images_batch): the image alone is enough.  The workgroup
// parses and validates the header with every check ghf_parse_header makes (written out: see section 1), fills the same tables,
// then finds the code boundaries itself: rounds of 256 subsequences of 512 bits, one per lane, settled by passes in
// which lane k restarts from where lane k - 1 landed until nothing moves at or in front of the first end mark (lane 0
// starts at an exactly known bit, so the fixed point is the true segmentation).  A scan of the lanes' symbol counts gives
// the output offsets; under kWrite the lanes decode once more into a 16 KiB stage that leaves slice by slice.
// ----------------------------------------------------------------------------------------------------------------------
// (kImgSubBits, kImgRoundBits, kImgStageBytes, kImgNone, kImgEndMark, kImgCutOff: ghf_batch_core.h)
struct BatchImagesLds {
  CodeTab t;
  // header phase: the raw symbol[] words, length / codeword by symbol, seen[], the raw start_pos / first_code words
  alignas(16) uint32_t stage[kImgStageBytes / 4 + 4];
  uint16_t over[2][kBatchThreads];  // bits each lane's last code runs past its subsequence; written in pass p, read in p + 1
  uint32_t mins[3][2];              // [pass % 3]{first lane whose start moved, first lane that met the end (mark) of the stream}
  uint32_t wave_tot[kBatchWaves];
  uint32_t stop_kind;
  unsigned long long kraft;
  uint32_t used;
  int bad;
};
static_assert(sizeof(BatchImagesLds) <= 40 * 1024, "four workgroups per CU");
static_assert(4 * (GHF_NSYM + 3) + 2 * 40 <= (int)kImgStageBytes / 4, "the header's scratch fits the stage");

template <bool kWrite>
__global__ __launch_bounds__(kBatchThreads) void k_decode_images_batch(BatchImagesParams P) {
  __shared__ BatchImagesLds S;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t item = blockIdx.x;
  const uint64_t stream_bytes = P.stream_bytes[item];
  const uint8_t* __restrict__ const stream = P.stream_ptrs[item];
  uint8_t* __restrict__ const out = kWrite ? P.out_ptrs[item] : nullptr;
  const uint64_t cap = kWrite ? P.out_caps[item] : ~0ull;
  uint32_t rounds = 0, passes = 0;
  auto finish = [&](int status, uint64_t n) {  // every lane of the workgroup takes the same exit
    if (tid == 0) {
      P.item_status[item] = status;
      P.out_bytes[item] = status == GHF_OK ? n : 0;
      if (P.stats && rounds) {
        atomicAdd(reinterpret_cast<unsigned long long*>(P.stats), (unsigned long long)rounds);
        atomicAdd(reinterpret_cast<unsigned long long*>(P.stats) + 1, (unsigned long long)passes);
      }
    }
  };
  if (!stream || (reinterpret_cast<uintptr_t>(stream) & 15u) || (kWrite && !out) || stream_bytes > P.max_stream_bytes)
    return finish(GHF_E_INVAL, 0);

  // ---- 1. the header: canonical_huff_encoder.cc:349-374 with the checks of ghf_parse_header ----
  // lengths are bounded before the header's size is trusted, the size against stream_bytes before the tables are read.
  // The rules are hdr_shape_ok, hdr_symbol_ok, hdr_len_ok and hdr_lone_end_mark_ok of ghf_code_rules.h, WRITTEN OUT here:
  // called as functions (any one of them, even len_bounds_ok alone) they re-lay this kernel, and both instantiations
  // measured 1 .. 7 % slower on the MI355X although the round loops kept the parent's opcodes (profiles/code_rules/
  // README.md).  In this form the listing is the parent's.  tests/header_cases.py holds one corrupted header per rule and
  // tests/test_gpu_batch_images.py asks that this copy and the host parser give the same verdicts.
  if (stream_bytes < kHeaderFixedBytes) return finish(GHF_E_FORMAT, 0);
  const uint32_t* __restrict__ const hw = reinterpret_cast<const uint32_t*>(stream);
  const uint32_t min_len_u = bswap32(hw[GHF_NSYM + 1]), max_len_u = bswap32(hw[GHF_NSYM + 2]);
  if (bswap32(hw[0]) != (uint32_t)GHF_NSYM || max_len_u < 1 || max_len_u > 32 || min_len_u < 1 || min_len_u > max_len_u)
    return finish(GHF_E_FORMAT, 0);
  const int min_len = (int)min_len_u, max_len = (int)max_len_u;
  const uint32_t hdr_bytes = header_bytes_for(max_len_u);
  if (stream_bytes < hdr_bytes) return finish(GHF_E_FORMAT, 0);

  uint32_t* const raw = S.stage;                     // symbol[] as stored
  uint32_t* const lenb = raw + (GHF_NSYM + 3);       // length by symbol
  uint32_t* const cwb = lenb + (GHF_NSYM + 3);       // codeword by symbol
  uint32_t* const seen = cwb + (GHF_NSYM + 3);
  uint32_t* const spraw = seen + (GHF_NSYM + 3);     // start_pos[0 .. 40) as stored; 0 outside [1, max_len]
  uint32_t* const fcraw = spraw + 40;                // first_code, likewise
  for (int i = tid; i < GHF_NSYM; i += kBatchThreads) {
    raw[i] = bswap32(hw[1 + i]);
    lenb[i] = 0;
    cwb[i] = 0;
    seen[i] = 0;
  }
  if (tid < 40) {
    const bool in = tid >= 1 && tid <= max_len;
    spraw[tid] = in ? bswap32(hw[GHF_NSYM + 3 + 2 * (tid - 1)]) : 0u;
    fcraw[tid] = in ? bswap32(hw[GHF_NSYM + 4 + 2 * (tid - 1)]) : 0u;
  }
  if (tid == 0) {
    S.kraft = 0;
    S.bad = 0;
    S.used = GHF_NSYM;
    for (int b = 0; b < 3; ++b) S.mins[b][0] = S.mins[b][1] = kImgNone;
  }
  __syncthreads();
  for (int i = tid; i < GHF_NSYM; i += kBatchThreads)
    if (raw[i] == kSymUnused) atomicMin(&S.used, (uint32_t)i);
  __syncthreads();
  const uint32_t used = S.used;  // used symbols are a prefix of symbol[], all distinct, the end mark among them
  {
    int b = 0;
    unsigned long long k = 0;
    for (int i = tid; i < GHF_NSYM; i += kBatchThreads) {
      const uint32_t s = raw[i];
      if ((uint32_t)i < used) {
        if (s >= (uint32_t)GHF_NSYM || atomicExch(&seen[s], 1u)) b = 1;
      } else if (s != 0xFFFFFFFFu) {
        b = 1;
      }
    }
    if (used == 1) {  // the empty stream of GHF_EMPTY_OK: the end mark alone, code "0" (not a complete code)
      if (tid == 0 && (max_len != 1 || fcraw[1] != 0 || spraw[1] != 0)) b = 1;
    } else {
      if (tid >= 1 && tid < min_len && fcraw[tid] != 1024u) b = 1;  // canonical_huff_encoder.cc:119-121
      if (tid >= min_len && tid <= max_len) {
        const uint32_t a = spraw[tid], e = tid < max_len ? spraw[tid + 1] : used;
        const unsigned long long fc = fcraw[tid];
        if (a > e || e > used || (tid == min_len && a != 0) || fc + (e - a) > (1ull << tid)) {
          b = 1;
        } else {
          k = (unsigned long long)(e - a) << (32 - tid);
          if (tid < max_len) {  // canonical_huff_encoder.cc:109-114: first_code[l] = (first_code[l + 1] + num[l + 1]) / 2
            const uint32_t nb = (tid + 1 < max_len ? spraw[tid + 2] : used) - spraw[tid + 1];
            if (fc != ((unsigned long long)fcraw[tid + 1] + nb) / 2) b = 1;
          } else if (fc != 0) {
            b = 1;
          }
        }
      }
    }
    if (k) atomicAdd(&S.kraft, k);
    if (b) atomicOr(&S.bad, 1);
  }
  __syncthreads();
  if (S.bad || !seen[GHF_NSYM - 1] || (used != 1 && S.kraft != (1ull << 32))) return finish(GHF_E_FORMAT, 0);
  // length / codeword by symbol, as ghf_parse_header rebuilds them: position k of symbol[] belongs to one length
  for (uint32_t k = tid; k < used; k += kBatchThreads) {
    for (int len = min_len; len <= max_len; ++len) {
      const uint32_t a = spraw[len], e = len < max_len ? spraw[len + 1] : used;
      if (k >= a && k < e) {
        lenb[raw[k]] = (uint32_t)len;
        cwb[raw[k]] = fcraw[len] + (k - a);
        break;
      }
    }
  }
  if (tid < 36) tab_load_row(S.t, tid, min_len, max_len, fcraw, spraw);
  for (int i = tid; i < GHF_NSYM; i += kBatchThreads) S.t.symbol[i] = tab_symbol(raw[i]);
  __syncthreads();
  if (P.codes) {
    ghf_code* const code = P.codes + item;
    for (int i = tid; i < GHF_NSYM; i += kBatchThreads) {
      code->length[i] = lenb[i];
      code->codeword[i] = cwb[i];
      code->symbol[i] = raw[i];
    }
    if (tid < 64) {
      code->first_code[tid] = tid < 40 ? fcraw[tid] : 0u;
      code->start_pos[tid] = tid < 40 ? spraw[tid] : 0u;
    }
    if (tid == 0) {
      code->min_len = min_len;
      code->max_len = max_len;
    }
  }
  if (used == 1) {  // nothing but the end mark "0" may follow
    const bool ok = stream_bytes > hdr_bytes && !(stream[hdr_bytes] & 0x80u);
    return finish(ok ? GHF_OK : GHF_E_CORRUPT, 0);
  }
  const int lb = max_len < kDecLutBitsMax ? max_len : kDecLutBitsMax;
  const int long_from = lb + 1 > min_len ? lb + 1 : min_len;
  tab_fill_lut(S.t, min_len, lb, tid, kBatchThreads);
  __syncthreads();  // (the header's scratch in the stage is dead from here on)

  // ---- 2. + 3. rounds of 256 subsequences ----
  const uint32_t end_bit = (uint32_t)stream_bytes * 8u;  // stream_bytes <= ghf_compress_bound(1 MiB): below 2^24 bytes
  uint32_t base = 8u * hdr_bytes;  // first bit of the round's subsequence 0
  uint32_t carry = 0;              // bits the previous round's last code runs into this one: lane 0's start, exact
  uint32_t total = 0;              // symbols of the rounds before this one
  uint32_t pb = 0, po = 0;         // pass % 3, pass % 2
#pragma unroll 1
  for (;;) {
    ++rounds;
    const uint32_t sub0 = base + (uint32_t)tid * kImgSubBits, sub_end = sub0 + kImgSubBits;
    uint32_t start = kImgNone, cnt = 0, stop = 0, over = 0;
    uint32_t round_passes = 0, first_stop;
#pragma unroll 1
    for (;;) {
      const uint32_t in = tid == 0 ? carry : round_passes == 0 ? 0u : (uint32_t)S.over[po][tid - 1];
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
          const uint32_t ent = batch_decode_one(S.t, cur.window(), lb, long_from, max_len);
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
      S.over[po ^ 1u][tid] = (uint16_t)over;
      const unsigned long long m_moved = __ballot(moved), m_stop = __ballot(stop != 0);
      if (lane == 0) {
        if (m_moved) atomicMin(&S.mins[pb][0], (uint32_t)(wave * 64 + __builtin_ctzll(m_moved)));
        if (m_stop) atomicMin(&S.mins[pb][1], (uint32_t)(wave * 64 + __builtin_ctzll(m_stop)));
      }
      const uint32_t nb = pb == 2 ? 0u : pb + 1;
      if (tid == 0) S.mins[nb][0] = S.mins[nb][1] = kImgNone;  // last read two barriers ago, next written behind this one
      __syncthreads();
      const uint32_t first_moved = S.mins[pb][0];
      first_stop = S.mins[pb][1];
      pb = nb;
      po ^= 1u;
      ++round_passes;
      // settled: nothing moved at or in front of the first stop -- and lanes 0 .. p are exact after pass p in any case
      if (first_moved == kImgNone || first_moved > first_stop || first_stop < round_passes) break;
    }
    passes += round_passes;
    const uint32_t mine = (uint32_t)tid <= first_stop ? cnt : 0u;  // (first_stop == kImgNone: every lane counts)
    const uint32_t incl = wave_incl_scan_u32(mine);
    if (lane == 63) S.wave_tot[wave] = incl;
    if ((uint32_t)tid == first_stop) S.stop_kind = stop;
    __syncthreads();
    uint32_t before = 0, round_total = 0;
#pragma unroll
    for (int w = 0; w < kBatchWaves; ++w) {
      const uint32_t t = S.wave_tot[w];
      before += w < wave ? t : 0u;
      round_total += t;
    }
    const uint32_t stop_kind = first_stop == kImgNone ? 0u : S.stop_kind;
    if (stop_kind == kImgCutOff) return finish(GHF_E_CORRUPT, 0);  // the stream ends before a whole end mark
    if ((uint64_t)total + round_total > cap) return finish(GHF_E_CAP, 0);  // before any store of the round
    if (kWrite) {
      const uint32_t rel = before + incl - mine;  // of the lane's first symbol in the round's output
      uint32_t i = 0;
      BatchCursor cur;
      if (mine) cur.seek(stream, stream_bytes, sub0 + start);
      uint8_t* const sb = reinterpret_cast<uint8_t*>(S.stage);
#pragma unroll 1
      for (uint32_t lo = 0; lo < round_total; lo += kImgStageBytes) {  // (min_len 1: a round holds up to 128 Ki symbols)
        while (i < mine && rel + i < lo + kImgStageBytes) {
          const uint32_t ent = batch_decode_one(S.t, cur.window(), lb, long_from, max_len);
          sb[rel + i - lo] = (uint8_t)ent;
          cur.skip(stream, stream_bytes, ent >> 9);
          ++i;
        }
        __syncthreads();
        const uint32_t rbytes = round_total - lo < kImgStageBytes ? round_total - lo : kImgStageBytes;
        batch_store_stage(out + total + lo, S.stage, rbytes, tid);
        __syncthreads();
      }
    }
    total += round_total;
    if (stop_kind == kImgEndMark) return finish(GHF_OK, total);
    carry = S.over[po][kBatchThreads - 1];
    base += kImgRoundBits;
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
void launch_decode_images_batch(const BatchImagesParams& p, uint32_t count, hipStream_t s) {
  if (count == 0) return;
  if (p.out_ptrs) hipLaunchKernelGGL(k_decode_images_batch<true>, dim3(count), dim3(kBatchThreads), 0, s, p);
  else hipLaunchKernelGGL(k_decode_images_batch<false>, dim3(count), dim3(kBatchThreads), 0, s, p);
}

}  // namespace ghf
