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
// (one workgroup per histogram of 257 counts: ghf_histogram_batch_planes has one per byte plane)
__global__ __launch_bounds__(256) void k_histogram_batch_finish(uint64_t* hists, uint32_t cover) {
  const int tid = threadIdx.x;
  uint64_t* const hist = hists + (size_t)blockIdx.x * GHF_NSYM;
  if (cover && hist[tid] == 0) hist[tid] = 1;
  if (tid == 0) hist[256] = 1;
}

// ----------------------------------------------------------------------------------------------------------------------
// compress: one workgroup per item runs batch_shared_compress_body (ghf_batch_core.h) over the item's bytes as they lie.
// ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBatchThreads) void k_compress_batch_shared(BatchSharedCompressParams P) {
  __shared__ BatchSharedCompressLds S;
  const uint32_t item = blockIdx.x;
  const BatchSharedSlot W = {P.code,      P.out_ptrs, P.out_caps,        P.out_bytes,     P.item_status,
                             P.chunk_bit, P.seg_bit,  P.blocks_per_item, P.segs_per_item, item};
  FlatItem it;
  it.in_ptrs = P.in_ptrs;
  it.in_bytes = P.in_bytes;
  it.max_item_bytes = P.max_item_bytes;
  it.item = item;
  batch_shared_compress_body(S, W, it);
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

  const int long_from = lb + 1 > min_len ? lb + 1 : min_len;
  batch_decode_segments(S, stream, stream_bytes, P.chunk_bit + (uint64_t)item * P.blocks_per_item,
                        P.seg_bit + (uint64_t)item * P.segs_per_item, n, out, lb, long_from, max_len, StoreFlat());
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
  launch_histogram_batch_finish(p.hist, 1, flags, s);
}
void launch_histogram_batch_finish(uint64_t* d_hists, uint32_t n_hists, uint32_t flags, hipStream_t s) {
  hipLaunchKernelGGL(k_histogram_batch_finish, dim3(n_hists), dim3(256), 0, s, d_hists, (uint32_t)((flags & GHF_HIST_COVER_ALL) != 0));
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
