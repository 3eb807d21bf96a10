// golden-huffman_amd/csrc/ghf_batch_planes.hip -- many small items of typed elements under one code PER BYTE PLANE
// (ghf_histogram_batch_planes, ghf_build_codes, ghf_compress_batch_planes_shared, ghf_decode_batch_planes_shared,
// ghf_decode_bodies_batch_planes_shared, include/ghf.h).
//
// ghf_batch_shared.hip puts one code under a batch of flat items; ghf_planes.hip gives the byte positions of the elements
// of ONE large buffer a .crs2 image each.  Here an item is a run of elements of E = 2, 4 or 8 bytes, plane p of it is the
// bytes in[p], in[p + E], .., and slot j = i * E + p holds the body of plane p of item i under codes[p]: exactly what
// k_compress_batch_shared writes for those bytes.  The planes are never materialised: the packer reads them out of the
// interleaved item (PlaneItem, ghf_batch_core.h) and the decoders write them into it (StorePlane).
#include "ghf_batch_core.h"
#include "ghf_build_code.h"
#include "ghf_code_rules.h"

namespace ghf {

// ----------------------------------------------------------------------------------------------------------------------
// histograms: k_histogram_batch's persistent grid with one bin set per plane.  Byte k of a lane's vector at item offset
// off (a multiple of 16, as E divides 16) belongs to plane k % E.  A u32 bin of plane p holds at most the plane's bytes
// counted since the last flush, kHistPlaneFlushBytes + GHF_BATCH_MAX_ITEM / E < 2^32.  hists[] is zeroed on the stream in
// front of the kernel; slot 256 and GHF_HIST_COVER_ALL are k_histogram_batch_finish's, one workgroup per plane.
// ----------------------------------------------------------------------------------------------------------------------
constexpr uint32_t kHistPlaneFlushBytes = 1u << 31;  // per plane
static_assert((uint64_t)kHistPlaneFlushBytes + GHF_BATCH_MAX_ITEM / 2 < (1ull << 32), "a u32 bin never wraps between two flushes");
// one resident round: 256 CUs x 8 workgroups of 4 waves, as k_histogram_batch; 4 at E = 8, whose 32 KiB of LDS let no more in
constexpr uint32_t hist_planes_grid(uint32_t elem_bytes) { return 256u * (elem_bytes == 8 ? 4u : 8u); }

template <int E>
__global__ __launch_bounds__(kBatchThreads) void k_histogram_batch_planes(BatchPlanesHistParams P) {
  __shared__ uint32_t bins[E][kBatchWaves][256];
  const int tid = threadIdx.x, wave = tid >> 6;
#pragma unroll
  for (int p = 0; p < E; ++p)
#pragma unroll
    for (int w = 0; w < kBatchWaves; ++w) bins[p][w][tid] = 0;
  __syncthreads();
  auto flush = [&]() {  // every lane of the workgroup takes it together; bin `tid` of every plane is this lane's from barrier to barrier
    __syncthreads();
#pragma unroll
    for (int p = 0; p < E; ++p) {
      unsigned long long c = 0;
#pragma unroll
      for (int w = 0; w < kBatchWaves; ++w) {
        c += bins[p][w][tid];
        bins[p][w][tid] = 0;
      }
      if (c) atomicAdd(reinterpret_cast<unsigned long long*>(P.hists) + p * GHF_NSYM + tid, c);
    }
    __syncthreads();
  };
  uint32_t counted = 0;  // bytes per plane since the last flush; the same in every lane
#pragma unroll 1
  for (uint32_t item = blockIdx.x; item < P.count; item += gridDim.x) {
    const uint64_t n64 = P.in_bytes[item];
    const uint8_t* __restrict__ const in = P.in_ptrs[item];
    if (n64 == 0 || n64 > P.max_item_bytes || !in || n64 % E) continue;  // ghf_compress_batch_planes_shared reports these
    const uint32_t n = (uint32_t)n64;
    const uint32_t mis = (uint32_t)reinterpret_cast<uintptr_t>(in) & 15u;
    for (uint32_t off = (uint32_t)tid * 16u; off < n; off += kBatchRoundSymbols) {
      const uint4 v = batch_load16(in, off, n, mis);
      const uint32_t cnt = n - off < 16u ? n - off : 16u;
#pragma unroll
      for (int k = 0; k < 16; ++k)
        if ((uint32_t)k < cnt) atomicAdd(&bins[k % E][wave][batch_byte(v, k)], 1u);
    }
    counted += n / E;
    if (counted > kHistPlaneFlushBytes) {
      flush();
      counted = 0;
    }
  }
  flush();
}

// ----------------------------------------------------------------------------------------------------------------------
// n exact code builds in one launch: one one-wave workgroup per code, each running build_code_body as k_build_code does
// (ghf_kernels.hip), on hists + 257 k into codes + k.  Failures latch at *status as ghf_build_code_ex latches them.
// ----------------------------------------------------------------------------------------------------------------------
template <bool LIMIT>
__global__ __launch_bounds__(64) void k_build_codes(const unsigned long long* __restrict__ hists, ghf_code* __restrict__ codes,
                                                    int* __restrict__ status, uint32_t empty_ok) {
  __shared__ HeapLds heap;
  __shared__ typename std::conditional<LIMIT, LimitLds, NoLimitLds>::type Q;
  __builtin_amdgcn_s_setprio(3);  // see k_build_code
  __shared__ CodeLds cl;
  __shared__ int s_ndata;
  build_code_body<LIMIT, true>(heap, Q, cl, s_ndata, HistCounts{hists + (size_t)blockIdx.x * GHF_NSYM}, codes + blockIdx.x, status,
                               empty_ok, threadIdx.x);
}

// ----------------------------------------------------------------------------------------------------------------------
// compress: one workgroup per slot runs batch_shared_compress_body (ghf_batch_core.h) over plane p of item i under
// codes[p].  The code's check is the slot's own, so an incomplete codes[p] refuses the slots of plane p alone.
// ----------------------------------------------------------------------------------------------------------------------
template <int E>
__global__ __launch_bounds__(kBatchThreads) void k_compress_batch_planes_shared(BatchPlanesCompressParams P) {
  __shared__ BatchSharedCompressLds S;
  const uint32_t slot = blockIdx.x, p = slot % E;
  const BatchSharedSlot W = {P.codes + p, P.out_ptrs, P.out_caps,        P.out_bytes,     P.item_status,
                             P.chunk_bit, P.seg_bit,  P.blocks_per_item, P.segs_per_item, slot};
  PlaneItem<E> it;
  it.in_ptrs = P.in_ptrs;
  it.in_bytes = P.in_bytes;
  it.max_item_bytes = P.max_item_bytes;
  it.slot = slot;
  batch_shared_compress_body(S, W, it);
}

// ----------------------------------------------------------------------------------------------------------------------
// The decoders: one workgroup per ITEM, taking its planes in turn -- status, size and the agreement of the planes are
// then the workgroup's own, without traffic between workgroups.  All E codes are vetted before the first store (so that a
// code that is not complete is reported on every item and nothing is written), then for each plane the CodeTab is filled
// and the round loop of the flat kernel runs with StorePlane as its way out of the stage.
// ----------------------------------------------------------------------------------------------------------------------
struct PlanesVetLds {
  unsigned long long kraft[GHF_PLANES_MAX];
  int bad;
};
// every lane of the workgroup; a barrier lies behind it.  -> all E codes are complete prefix codes (ghf_code_rules.h, section 2)
template <int E>
__device__ __forceinline__ bool planes_codes_ok(PlanesVetLds& V, const ghf_code* __restrict__ codes, int tid) {
  if (tid < E) V.kraft[tid] = 0;
  if (tid == 0) V.bad = 0;
  __syncthreads();
#pragma unroll 1
  for (int p = 0; p < E; ++p) {
    const int max_len = codes[p].max_len, min_len = codes[p].min_len;
    if (!len_bounds_ok(min_len, max_len)) {
      if (tid == 0) V.bad = 1;  // (the same in every lane)
      continue;
    }
    unsigned long long k = 0;
    if (!code_share_ok(codes + p, min_len, max_len, tid, kBatchThreads, &k)) atomicOr(&V.bad, 1);
    if (k) atomicAdd(&V.kraft[p], k);
  }
  __syncthreads();
  bool ok = V.bad == 0;
#pragma unroll
  for (int p = 0; p < E; ++p) ok &= V.kraft[p] == (1ull << 32);
  return ok;
}

struct BatchPlanesDecodeLds {
  CodeTab t;  // the tables of the plane in work
  alignas(16) uint32_t stage[kBatchDecRoundBytes / 4 + 4];
  PlanesVetLds vet;
  int err;
};
static_assert(sizeof(BatchPlanesDecodeLds) <= 40 * 1024, "four workgroups per CU");

template <int E>
__global__ __launch_bounds__(kBatchThreads) void k_decode_batch_planes_shared(BatchPlanesDecodeParams P) {
  __shared__ BatchPlanesDecodeLds S;
  const int tid = threadIdx.x;
  const uint32_t item = blockIdx.x;
  auto finish = [&](int status, uint64_t bytes) {  // every lane of the workgroup takes the same exit
    if (tid == 0) {
      P.item_status[item] = status;
      P.out_bytes[item] = bytes;
    }
  };
  if (tid == 0) S.err = 0;
  if (!planes_codes_ok<E>(S.vet, P.codes, tid)) return finish(GHF_E_FORMAT, 0);

  const uint64_t n64 = P.n_elems[item];
  uint8_t* __restrict__ const out = P.out_ptrs[item];
  if (n64 == 0) return finish(GHF_E_EMPTY, 0);
  bool inval = n64 > P.max_plane_symbols || !out;
#pragma unroll
  for (int p = 0; p < E; ++p) {
    const uint8_t* const sp = P.stream_ptrs[(size_t)item * E + p];
    inval |= !sp || (reinterpret_cast<uintptr_t>(sp) & 15u);
  }
  if (inval) return finish(GHF_E_INVAL, 0);
  if (n64 * E > P.out_caps[item]) return finish(GHF_E_CAP, 0);  // (n64 <= 2^20)
  const uint32_t n = (uint32_t)n64;

#pragma unroll 1
  for (uint32_t p = 0; p < E; ++p) {
    const size_t slot = (size_t)item * E + p;
    int lb, long_from, max_len;
    batch_code_tables(S.t, P.codes + p, tid, lb, long_from, max_len);
    batch_decode_segments(S, P.stream_ptrs[slot], P.stream_bytes[slot], P.chunk_bit + slot * P.blocks_per_item,
                          P.seg_bit + slot * P.segs_per_item, n, out, lb, long_from, max_len, StorePlane<E>{p});
  }
  const bool ok = S.err == 0;  // (a barrier closes the last round)
  finish(ok ? GHF_OK : GHF_E_CORRUPT, ok ? (uint64_t)n * E : 0);
}

struct BatchPlanesBodiesLds {
  CodeTab t;
  alignas(16) uint32_t stage[kImgStageBytes / 4 + 4];
  BatchRoundsLds r;
  PlanesVetLds vet;
};
static_assert(sizeof(BatchPlanesBodiesLds) <= 40 * 1024, "four workgroups per CU");

template <int E, bool kWrite>
__global__ __launch_bounds__(kBatchThreads) void k_decode_bodies_batch_planes_shared(BatchPlanesBodiesParams P) {
  __shared__ BatchPlanesBodiesLds S;
  const int tid = threadIdx.x;
  const uint32_t item = blockIdx.x;
  uint32_t rounds = 0, passes = 0, n = 0;
  int status = planes_codes_ok<E>(S.vet, P.codes, tid) ? GHF_OK : GHF_E_FORMAT;  // the same in every lane, as is all below
  uint8_t* __restrict__ out = nullptr;
  uint64_t cap = ~0ull;  // a plane's cap, in symbols
  if (status == GHF_OK) {
    bool inval = false;
    if (kWrite) {
      out = P.out_ptrs[item];
      cap = P.out_caps[item] / E;
      inval = !out;
    }
#pragma unroll
    for (int p = 0; p < E; ++p) {
      const uint8_t* const sp = P.stream_ptrs[(size_t)item * E + p];
      inval |= !sp || (reinterpret_cast<uintptr_t>(sp) & 15u) || P.stream_bytes[(size_t)item * E + p] > P.max_stream_bytes;
    }
    if (inval) status = GHF_E_INVAL;
  }
#pragma unroll 1
  for (uint32_t p = 0; p < E && status == GHF_OK; ++p) {
    const size_t slot = (size_t)item * E + p;
    int lb, long_from, max_len;
    if (tid == 0) batch_rounds_init(S.r);  // (the barriers of batch_code_tables lie between this and the rounds)
    batch_code_tables(S.t, P.codes + p, tid, lb, long_from, max_len);
    uint32_t total = 0;  // stream_bytes <= ghf_compress_batch_shared_bound(1 MiB): every bit offset fits 32 bits
    status = batch_decode_rounds<kWrite>(S.t, S.stage, S.r, P.stream_ptrs[slot], P.stream_bytes[slot], 0u, cap, out, lb, long_from,
                                         max_len, &total, rounds, passes, StorePlane<E>{p});
    if (status == GHF_OK && p != 0 && total != n) status = GHF_E_CORRUPT;  // the planes of one item hold the same number of symbols
    n = total;
  }
  if (tid == 0) {
    P.item_status[item] = status;
    P.out_bytes[item] = status == GHF_OK ? (uint64_t)n * E : 0;
    if (P.stats && rounds) {
      atomicAdd(reinterpret_cast<unsigned long long*>(P.stats), (unsigned long long)rounds);
      atomicAdd(reinterpret_cast<unsigned long long*>(P.stats) + 1, (unsigned long long)passes);
    }
  }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------
#define GHF_PLANES_DISPATCH(E_, CALL) \
  do {                                \
    if ((E_) == 2) { CALL(2); }       \
    else if ((E_) == 4) { CALL(4); }  \
    else { CALL(8); }                 \
  } while (0)

void launch_histogram_batch_planes(const BatchPlanesHistParams& p, uint32_t elem_bytes, uint32_t flags, hipStream_t s) {
  if (p.count == 0) return;
  (void)hipMemsetAsync(p.hists, 0, (size_t)elem_bytes * GHF_NSYM * sizeof(uint64_t), s);
  const uint32_t grid = p.count < hist_planes_grid(elem_bytes) ? p.count : hist_planes_grid(elem_bytes);
#define GHF_CALL(E) hipLaunchKernelGGL(k_histogram_batch_planes<E>, dim3(grid), dim3(kBatchThreads), 0, s, p)
  GHF_PLANES_DISPATCH(elem_bytes, GHF_CALL);
#undef GHF_CALL
  launch_histogram_batch_finish(p.hists, elem_bytes, flags, s);
}

void launch_build_codes(const uint64_t* d_hists, uint32_t n_codes, ghf_code* d_codes, int* d_status, uint32_t flags, hipStream_t s) {
  const unsigned long long* const h = reinterpret_cast<const unsigned long long*>(d_hists);
  if (flags & GHF_CODE_LIMIT) hipLaunchKernelGGL(k_build_codes<true>, dim3(n_codes), dim3(64), 0, s, h, d_codes, d_status, flags & GHF_EMPTY_OK);
  else hipLaunchKernelGGL(k_build_codes<false>, dim3(n_codes), dim3(64), 0, s, h, d_codes, d_status, flags & GHF_EMPTY_OK);
}

void launch_compress_batch_planes_shared(const BatchPlanesCompressParams& p, uint32_t count, uint32_t elem_bytes, hipStream_t s) {
  if (count == 0) return;
  const dim3 grid(count * elem_bytes);
#define GHF_CALL(E) hipLaunchKernelGGL(k_compress_batch_planes_shared<E>, grid, dim3(kBatchThreads), 0, s, p)
  GHF_PLANES_DISPATCH(elem_bytes, GHF_CALL);
#undef GHF_CALL
}

void launch_decode_batch_planes_shared(const BatchPlanesDecodeParams& p, uint32_t count, uint32_t elem_bytes, hipStream_t s) {
  if (count == 0) return;
#define GHF_CALL(E) hipLaunchKernelGGL(k_decode_batch_planes_shared<E>, dim3(count), dim3(kBatchThreads), 0, s, p)
  GHF_PLANES_DISPATCH(elem_bytes, GHF_CALL);
#undef GHF_CALL
}

void launch_decode_bodies_batch_planes_shared(const BatchPlanesBodiesParams& p, uint32_t count, uint32_t elem_bytes, hipStream_t s) {
  if (count == 0) return;
#define GHF_CALL(E)                                                                                                                \
  if (p.out_ptrs) hipLaunchKernelGGL((k_decode_bodies_batch_planes_shared<E, true>), dim3(count), dim3(kBatchThreads), 0, s, p); \
  else hipLaunchKernelGGL((k_decode_bodies_batch_planes_shared<E, false>), dim3(count), dim3(kBatchThreads), 0, s, p)
  GHF_PLANES_DISPATCH(elem_bytes, GHF_CALL);
#undef GHF_CALL
}
#undef GHF_PLANES_DISPATCH

}  // namespace ghf
