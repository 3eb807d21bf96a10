// golden-huffman_amd/csrc/ghf_batch_shared.hip -- many small items under ONE code (ghf_histogram_batch,
// ghf_compress_batch_shared, ghf_decode_batch_shared, ghf_decode_bodies_batch_shared, include/ghf.h; DESIGN.md
// sections 12 and 13).
//
// ghf_batch.hip gives every item a code of its own: a header of 1040 + 8 max_len bytes per image, 3604 bytes of tables per
// item for the decoder and a one-wavefront code build inside every workgroup.  Here the code comes from the caller (built
// from the batch's histogram, from a sample, or parsed from a stored header) and an item's output is its BODY alone:
// its codes from bit 0, the end mark, 1-bits up to the byte.  header(code) || body is a standalone .crs2 image.
#include "ghf_batch_core.h"
#include "ghf_code_rules.h"

namespace ghf {

// ----------------------------------------------------------------------------------------------------------------------
// histogram of the whole batch: a persistent grid, every workgroup strides over the items and counts into one u32 LDS
// replica per wave (phase 1 of k_compress_batch); its 256 sums leave with 64-bit atomic adds at its end -- and earlier
// whenever it has counted more than kHistFlushBytes since its last flush, so that a u32 bin holds at most
// kHistFlushBytes + GHF_BATCH_MAX_ITEM < 2^32.  hist[] is zeroed on the stream in front of the kernel; the end mark's
// count and GHF_HIST_COVER_ALL are k_histogram_batch_finish's, a launch behind it (the stream orders the atomics).
// ----------------------------------------------------------------------------------------------------------------------
constexpr uint32_t kHistFlushBytes = 1u << 31;
static_assert((uint64_t)kHistFlushBytes + GHF_BATCH_MAX_ITEM < (1ull << 32), "a u32 bin never wraps between two flushes");
constexpr uint32_t kHistBatchGrid = 256 * 8;  // one resident round: 256 CUs x 8 workgroups of 4 waves and 4 KiB of LDS

__global__ __launch_bounds__(kBatchThreads) void k_histogram_batch(BatchHistParams P) {
  __shared__ uint32_t bins[kBatchWaves][256];
  const int tid = threadIdx.x, wave = tid >> 6;
#pragma unroll
  for (int w = 0; w < kBatchWaves; ++w) bins[w][tid] = 0;
  __syncthreads();
  auto flush = [&]() {  // every lane of the workgroup takes it together; bin `tid` is this lane's from barrier to barrier
    __syncthreads();
    unsigned long long c = 0;
#pragma unroll
    for (int w = 0; w < kBatchWaves; ++w) {
      c += bins[w][tid];
      bins[w][tid] = 0;
    }
    if (c) atomicAdd(reinterpret_cast<unsigned long long*>(P.hist) + tid, c);
    __syncthreads();
  };
  uint32_t counted = 0;  // bytes since the last flush; the same in every lane
#pragma unroll 1
  for (uint32_t item = blockIdx.x; item < P.count; item += gridDim.x) {
    const uint64_t n64 = P.in_bytes[item];
    const uint8_t* __restrict__ const in = P.in_ptrs[item];
    if (n64 == 0 || n64 > P.max_item_bytes || !in) continue;  // ghf_compress_batch_shared reports these
    const uint32_t n = (uint32_t)n64;
    const uint32_t mis = (uint32_t)reinterpret_cast<uintptr_t>(in) & 15u;
    for (uint32_t off = (uint32_t)tid * 16u; off < n; off += kBatchRoundSymbols) {
      const uint4 v = batch_load16(in, off, n, mis);
      const uint32_t cnt = n - off < 16u ? n - off : 16u;
#pragma unroll
      for (int k = 0; k < 16; ++k)
        if ((uint32_t)k < cnt) atomicAdd(&bins[wave][batch_byte(v, k)], 1u);
    }
    counted += n;
    if (counted > kHistFlushBytes) {
      flush();
      counted = 0;
    }
  }
  flush();
}

// behind k_histogram_batch on the same stream: the end mark counts once (include/encoder.h:123-129); cover: no count stays 0
__global__ __launch_bounds__(256) void k_histogram_batch_finish(uint64_t* hist, uint32_t cover) {
  const int tid = threadIdx.x;
  if (cover && hist[tid] == 0) hist[tid] = 1;
  if (tid == 0) hist[256] = 1;
}

// ----------------------------------------------------------------------------------------------------------------------
// compress: one workgroup per item.  The shared code is checked once per workgroup (the rules k_decode_batch applies to
// an item's tables), a pricing pass gives the body's exact size before the first store, then the round loop of
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

__global__ __launch_bounds__(kBatchThreads) void k_compress_batch_shared(BatchSharedCompressParams P) {
  __shared__ BatchSharedCompressLds S;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t item = blockIdx.x;
  const ghf_code* __restrict__ const code = P.code;
  auto finish = [&](int status, uint64_t bytes) {  // every lane of the workgroup takes the same exit
    if (tid == 0) {
      P.item_status[item] = status;
      P.out_bytes[item] = bytes;
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

  const uint64_t n64 = P.in_bytes[item];
  const uint8_t* __restrict__ const in = P.in_ptrs[item];
  uint8_t* __restrict__ const out = P.out_ptrs[item];
  if (n64 == 0) return finish(GHF_E_EMPTY, 0);
  if (n64 > P.max_item_bytes || !in || !out || (reinterpret_cast<uintptr_t>(out) & 15u)) return finish(GHF_E_INVAL, 0);
  const uint32_t n = (uint32_t)n64;
  const uint32_t mis = (uint32_t)reinterpret_cast<uintptr_t>(in) & 15u;

  // ---- 2. the price: the sum of the lengths, and whether a byte value without a code occurs ----
  {
    uint32_t bits = 0;
    bool none = false;
    for (uint32_t off = (uint32_t)tid * 16u; off < n; off += kBatchRoundSymbols) {
      const uint4 v = batch_load16(in, off, n, mis);
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
  if (body_bytes > P.out_caps[item]) return finish(GHF_E_CAP, 0);

  uint64_t* const chunk_bit = P.chunk_bit ? P.chunk_bit + (uint64_t)item * P.blocks_per_item : nullptr;
  uint32_t* const seg_bit = P.seg_bit ? P.seg_bit + (uint64_t)item * P.segs_per_item : nullptr;

  // ---- 4. the round loop of k_compress_batch from body bit 0: one side-car block per round ----
  uint32_t B = 0;  // body bit of the next code
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

// ----------------------------------------------------------------------------------------------------------------------
// decode: the body of k_decode_batch with one code for every item and bodies that start at bit 0.  The code is vetted
// before the item is looked at, so a code that is not complete is reported on every item.
// ----------------------------------------------------------------------------------------------------------------------
struct BatchSharedDecodeLds {
  CodeTab t;  // the shared code's decode tables (ghf_code_rules.h)
  alignas(16) uint32_t stage[kBatchDecRoundBytes / 4 + 4];
  unsigned long long kraft;
  int bad;
  int err;
};
static_assert(sizeof(BatchSharedDecodeLds) <= 40 * 1024, "four workgroups per CU");

__global__ __launch_bounds__(kBatchThreads) void k_decode_batch_shared(BatchSharedDecodeParams P) {
  __shared__ BatchSharedDecodeLds S;
  const int tid = threadIdx.x;
  const uint32_t item = blockIdx.x;
  const ghf_code* __restrict__ const code = P.code;
  auto finish = [&](int status, uint64_t bytes) {
    if (tid == 0) {
      P.item_status[item] = status;
      P.out_bytes[item] = bytes;
    }
  };
  // a complete prefix code (ghf_code_rules.h, section 2), and its tables
  const int max_len = code->max_len, min_len = code->min_len;
  if (!len_bounds_ok(min_len, max_len)) return finish(GHF_E_FORMAT, 0);
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
  if (S.bad || S.kraft != (1ull << 32)) return finish(GHF_E_FORMAT, 0);

  const uint64_t n64 = P.n_symbols[item];
  const uint64_t stream_bytes = P.stream_bytes[item];
  const uint8_t* __restrict__ const stream = P.stream_ptrs[item];
  uint8_t* __restrict__ const out = P.out_ptrs[item];
  if (n64 == 0) return finish(GHF_E_EMPTY, 0);
  if (n64 > P.max_item_bytes || !stream || !out || (reinterpret_cast<uintptr_t>(stream) & 15u)) return finish(GHF_E_INVAL, 0);
  if (n64 > P.out_caps[item]) return finish(GHF_E_CAP, 0);
  const uint32_t n = (uint32_t)n64;

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
  const bool ok = S.err == 0;
  finish(ok ? GHF_OK : GHF_E_CORRUPT, ok ? n : 0);
}

// ----------------------------------------------------------------------------------------------------------------------
// decode of bodies that come with nothing else (ghf_decode_bodies_batch_shared): the front of
// k_decode_batch_shared (the code is vetted before the item is looked at), then the round loop of k_decode_images_batch
// from body bit 0 (batch_decode_rounds, ghf_batch_core.h): the workgroup finds the code boundaries and the size itself.
// ----------------------------------------------------------------------------------------------------------------------
struct BatchSharedBodiesLds {
  CodeTab t;  // the shared code's decode tables (ghf_code_rules.h)
  alignas(16) uint32_t stage[kImgStageBytes / 4 + 4];
  BatchRoundsLds r;
  unsigned long long kraft;
  int bad;
};
static_assert(sizeof(BatchSharedBodiesLds) <= 40 * 1024, "four workgroups per CU");

template <bool kWrite>
__global__ __launch_bounds__(kBatchThreads) void k_decode_bodies_batch_shared(BatchSharedBodiesParams P) {
  __shared__ BatchSharedBodiesLds S;
  const int tid = threadIdx.x;
  const uint32_t item = blockIdx.x;
  const ghf_code* __restrict__ const code = P.code;
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
  // a complete prefix code (ghf_code_rules.h, section 2), and its tables
  const int max_len = code->max_len, min_len = code->min_len;
  if (!len_bounds_ok(min_len, max_len)) return finish(GHF_E_FORMAT, 0);
  if (tid == 0) {
    S.kraft = 0;
    S.bad = 0;
    batch_rounds_init(S.r);
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
  if (S.bad || S.kraft != (1ull << 32)) return finish(GHF_E_FORMAT, 0);

  const uint64_t stream_bytes = P.stream_bytes[item];
  const uint8_t* __restrict__ const stream = P.stream_ptrs[item];
  uint8_t* __restrict__ const out = kWrite ? P.out_ptrs[item] : nullptr;
  const uint64_t cap = kWrite ? P.out_caps[item] : ~0ull;
  if (!stream || (reinterpret_cast<uintptr_t>(stream) & 15u) || (kWrite && !out) || stream_bytes > P.max_stream_bytes)
    return finish(GHF_E_INVAL, 0);

  const int lb = max_len < kDecLutBitsMax ? max_len : kDecLutBitsMax;
  const int long_from = lb + 1 > min_len ? lb + 1 : min_len;
  tab_fill_lut(S.t, min_len, lb, tid, kBatchThreads);
  __syncthreads();

  uint32_t total = 0;  // stream_bytes <= ghf_compress_batch_shared_bound(1 MiB): every bit offset fits 32 bits
  const int status = batch_decode_rounds<kWrite>(S.t, S.stage, S.r, stream, stream_bytes, 0u, cap, out, lb, long_from, max_len,
                                                 &total, rounds, passes);
  finish(status, total);
}

void launch_histogram_batch(const BatchHistParams& p, uint32_t flags, hipStream_t s) {
  if (p.count == 0) return;
  (void)hipMemsetAsync(p.hist, 0, 256 * sizeof(uint64_t), s);  // (slot 256 is the finish kernel's)
  const uint32_t grid = p.count < kHistBatchGrid ? p.count : kHistBatchGrid;
  hipLaunchKernelGGL(k_histogram_batch, dim3(grid), dim3(kBatchThreads), 0, s, p);
  hipLaunchKernelGGL(k_histogram_batch_finish, dim3(1), dim3(256), 0, s, p.hist, (uint32_t)((flags & GHF_HIST_COVER_ALL) != 0));
}
void launch_compress_batch_shared(const BatchSharedCompressParams& p, uint32_t count, hipStream_t s) {
  if (count == 0) return;
  hipLaunchKernelGGL(k_compress_batch_shared, dim3(count), dim3(kBatchThreads), 0, s, p);
}
void launch_decode_batch_shared(const BatchSharedDecodeParams& p, uint32_t count, hipStream_t s) {
  if (count == 0) return;
  hipLaunchKernelGGL(k_decode_batch_shared, dim3(count), dim3(kBatchThreads), 0, s, p);
}

void launch_decode_bodies_batch_shared(const BatchSharedBodiesParams& p, uint32_t count, hipStream_t s) {
  if (count == 0) return;
  if (p.out_ptrs) hipLaunchKernelGGL(k_decode_bodies_batch_shared<true>, dim3(count), dim3(kBatchThreads), 0, s, p);
  else hipLaunchKernelGGL(k_decode_bodies_batch_shared<false>, dim3(count), dim3(kBatchThreads), 0, s, p);
}

}  // namespace ghf
