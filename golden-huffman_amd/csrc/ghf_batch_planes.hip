// golden-huffman_amd/csrc/ghf_batch_planes.hip -- many small items of typed elements under one code PER BYTE PLANE
// (ghf_histogram_batch_planes, ghf_build_codes, ghf_compress_batch_planes_shared, ghf_decode_batch_planes_shared,
// ghf_decode_bodies_batch_planes_shared, include/ghf.h), and the same calls with some planes stored
// raw (ghf_batch_planes_raw_auto, ghf_compress_batch_planes_forms, ghf_decode_batch_planes_forms,
// ghf_decode_bodies_batch_planes_forms).
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

// ----------------------------------------------------------------------------------------------------------------------
// Planes in two forms: bit p of `raw` (a kernel argument: the same in every wave, an SGPR) says
// that plane p of the batch is stored as it is -- slot j = i * E + p holds the n bytes of the plane, nothing else.  A
// dense slot is what the kernels above write and read, byte for byte; codes[p] of a raw plane is never read.  The
// kernels above stay as they are: these are their plane loops with the raw branch in front of the table fill.  (One body
// per pair over <E, kForms> was built and lost timing rows to these written-out forms: profiles/batch_planes_bodies/README.md;
// tests/test_gpu_batch_planes_twins.py holds each pair to the same verdicts.)
// ----------------------------------------------------------------------------------------------------------------------
// which planes are raw: plane p is when sum hist[p][s] * length[p][s] >= 8 * sum hist[p][s] over s < 256 and the right
// side is not 0 (64-bit integers; the end mark is not counted): then its bodies, each rounded up behind an end mark, never
// store less than its bytes.  A code whose lengths are out of bounds (ghf_code_rules.h) leaves its plane dense: the
// packer reports that code.  One workgroup; lane s takes byte value s.
__global__ __launch_bounds__(kBatchThreads) void k_batch_planes_raw_auto(const unsigned long long* __restrict__ hists,
                                                                         const ghf_code* __restrict__ codes, uint32_t elem_bytes,
                                                                         uint32_t* __restrict__ raw_planes) {
  __shared__ unsigned long long s_bits[GHF_PLANES_MAX], s_syms[GHF_PLANES_MAX];
  const int tid = threadIdx.x;
  if (tid < GHF_PLANES_MAX) s_bits[tid] = s_syms[tid] = 0;
  __syncthreads();
  for (uint32_t p = 0; p < elem_bytes; ++p) {
    const unsigned long long h = hists[(size_t)p * GHF_NSYM + tid];
    if (h) {
      atomicAdd(&s_bits[p], h * codes[p].length[tid]);
      atomicAdd(&s_syms[p], h);
    }
  }
  __syncthreads();
  if (tid == 0) {
    uint32_t mask = 0;
    for (uint32_t p = 0; p < elem_bytes; ++p)
      if (len_bounds_ok(codes[p].min_len, codes[p].max_len) && s_syms[p] != 0 && s_bits[p] >= 8ull * s_syms[p]) mask |= 1u << p;
    *raw_planes = mask;
  }
}

// Which slot workgroup b of the forms packer takes: the dense slots first, item by item, then the raw ones.  Workgroups go
// to the XCDs in turn (b mod 8), so with slot = b the dense slots of bf16 under mask 0b01 -- the odd ones -- would all land
// on four of the eight XCDs and those of fp32 under 0b0111 on two: the packer then takes as long as with every plane dense
// (measured so: 0.99 and 1.01 of the parent).  In this order every XCD gets its share of both kinds, and the long
// workgroups start first.  raw == 0: slot = b.  All scalar: b, count and raw are the same in every lane.
template <int E>
__device__ __forceinline__ uint32_t forms_slot_of(uint32_t b, uint32_t count, uint32_t raw) {
  const uint32_t dense = ~raw & ((1u << E) - 1u), nd = (uint32_t)__builtin_popcount(dense);
  uint32_t planes = dense, per = nd;
  if (b >= count * nd) {
    b -= count * nd;
    planes = raw;
    per = E - nd;
  }
  const uint32_t item = b / per;
  uint32_t k = b % per, p = 0;
#pragma unroll
  for (uint32_t q = 0; q < E; ++q) {  // the k-th plane of `planes`
    if (planes >> q & 1u) {
      if (k == 0) p = q;
      --k;
    }
  }
  return item * E + p;
}

template <int E>
__global__ __launch_bounds__(kBatchThreads) void k_compress_batch_planes_forms(BatchPlanesCompressParams P, uint32_t raw) {
  __shared__ BatchSharedCompressLds S;
  const uint32_t slot = forms_slot_of<E>(blockIdx.x, gridDim.x / E, raw), p = slot % E;
  const BatchSharedSlot W = {P.codes + p, P.out_ptrs, P.out_caps,        P.out_bytes,     P.item_status,
                             P.chunk_bit, P.seg_bit,  P.blocks_per_item, P.segs_per_item, slot};
  PlaneItem<E> it;
  it.in_ptrs = P.in_ptrs;
  it.in_bytes = P.in_bytes;
  it.max_item_bytes = P.max_item_bytes;
  it.slot = slot;
  if (raw >> p & 1u) batch_raw_compress_body(W, it);  // (the same in every lane of the workgroup)
  else batch_shared_compress_body(S, W, it);
}

// planes_codes_ok over the dense planes alone: the code of a raw plane is not looked at
template <int E>
__device__ __forceinline__ bool planes_dense_codes_ok(PlanesVetLds& V, const ghf_code* __restrict__ codes, uint32_t raw, int tid) {
  if (tid < E) V.kraft[tid] = 0;
  if (tid == 0) V.bad = 0;
  __syncthreads();
#pragma unroll 1
  for (int p = 0; p < E; ++p) {
    if (raw >> p & 1u) continue;  // (the same in every lane)
    const int max_len = codes[p].max_len, min_len = codes[p].min_len;
    if (!len_bounds_ok(min_len, max_len)) {
      if (tid == 0) V.bad = 1;
      continue;
    }
    unsigned long long k = 0;
    if (!code_share_ok(codes + p, min_len, max_len, tid, kBatchThreads, &k)) atomicOr(&V.bad, 1);
    if (k) atomicAdd(&V.kraft[p], k);
  }
  __syncthreads();
  bool ok = V.bad == 0;
#pragma unroll
  for (int p = 0; p < E; ++p) ok &= (raw >> p & 1u) || V.kraft[p] == (1ull << 32);
  return ok;
}

// the live side-car decoder.  A raw slot holds exactly n_elems bytes (GHF_E_CORRUPT otherwise, seen for all raw planes of
// the item before its first store); its side-car slice is not read.
template <int E>
__global__ __launch_bounds__(kBatchThreads) void k_decode_batch_planes_forms(BatchPlanesDecodeParams P, uint32_t raw) {
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
  if (!planes_dense_codes_ok<E>(S.vet, P.codes, raw, tid)) return finish(GHF_E_FORMAT, 0);

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
  bool differ = false;
#pragma unroll
  for (int p = 0; p < E; ++p) differ |= (raw >> p & 1u) && P.stream_bytes[(size_t)item * E + p] != n64;
  if (differ) return finish(GHF_E_CORRUPT, 0);

#pragma unroll 1
  for (uint32_t p = 0; p < E; ++p) {
    const size_t slot = (size_t)item * E + p;
    if (raw >> p & 1u) {
      batch_raw_plane_copy<E>(S.stage, (uint32_t)kBatchDecRoundBytes, P.stream_ptrs[slot], n, out, p, tid);
      continue;
    }
    int lb, long_from, max_len;
    batch_code_tables(S.t, P.codes + p, tid, lb, long_from, max_len);
    batch_decode_segments(S, P.stream_ptrs[slot], P.stream_bytes[slot], P.chunk_bit + slot * P.blocks_per_item,
                          P.seg_bit + slot * P.segs_per_item, n, out, lb, long_from, max_len, StorePlane<E>{p});
  }
  __syncthreads();  // (S.err: the last plane may have been a raw one)
  const bool ok = S.err == 0;
  finish(ok ? GHF_OK : GHF_E_CORRUPT, ok ? (uint64_t)n * E : 0);
}

// the bodies-only decoder.  A raw slot's symbol count IS its size: the counts of the raw planes are held against their
// bounds, the cap and each other before the first store, and an item whose planes are all raw decodes from them alone.
template <int E, bool kWrite>
__global__ __launch_bounds__(kBatchThreads) void k_decode_bodies_batch_planes_forms(BatchPlanesBodiesParams P, uint32_t raw) {
  __shared__ BatchPlanesBodiesLds S;
  const int tid = threadIdx.x;
  const uint32_t item = blockIdx.x;
  uint32_t rounds = 0, passes = 0, n = 0;
  int status = planes_dense_codes_ok<E>(S.vet, P.codes, raw, tid) ? GHF_OK : GHF_E_FORMAT;  // the same in every lane, as is all below
  uint8_t* out = nullptr;
  uint64_t cap = ~0ull;  // a plane's cap, in symbols
  bool have = false;     // n holds the count of a plane of this item
  if (status == GHF_OK) {
    bool inval = false;
    if (kWrite) {
      out = P.out_ptrs[item];
      cap = P.out_caps[item] / E;
      inval = !out;
    }
    bool differ = false;
#pragma unroll
    for (int p = 0; p < E; ++p) {
      const uint8_t* const sp = P.stream_ptrs[(size_t)item * E + p];
      const uint64_t sb = P.stream_bytes[(size_t)item * E + p];
      inval |= !sp || (reinterpret_cast<uintptr_t>(sp) & 15u);
      if (raw >> p & 1u) {
        inval |= !batch_raw_count_ok<E>(sb);
        differ |= have && (uint32_t)sb != n;
        if (!have) n = (uint32_t)sb;
        have = true;
      } else {
        inval |= sb > P.max_stream_bytes;
      }
    }
    if (inval) status = GHF_E_INVAL;
    else if (have && n > cap) status = GHF_E_CAP;  // before any store of a raw plane
    else if (differ) status = GHF_E_CORRUPT;
  }
#pragma unroll 1
  for (uint32_t p = 0; p < E && status == GHF_OK; ++p) {
    const size_t slot = (size_t)item * E + p;
    if (raw >> p & 1u) {
      if (kWrite) batch_raw_plane_copy<E>(S.stage, kImgStageBytes, P.stream_ptrs[slot], n, out, p, tid);
      continue;
    }
    int lb, long_from, max_len;
    if (tid == 0) batch_rounds_init(S.r);  // (the barriers of batch_code_tables lie between this and the rounds)
    batch_code_tables(S.t, P.codes + p, tid, lb, long_from, max_len);
    uint32_t total = 0;  // stream_bytes <= ghf_compress_batch_shared_bound(1 MiB): every bit offset fits 32 bits
    status = batch_decode_rounds<kWrite>(S.t, S.stage, S.r, P.stream_ptrs[slot], P.stream_bytes[slot], 0u, cap, out, lb, long_from,
                                         max_len, &total, rounds, passes, StorePlane<E>{p});
    if (status == GHF_OK && have && total != n) status = GHF_E_CORRUPT;  // the planes of one item hold the same number of symbols
    n = total;
    have = true;
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
void launch_histogram_batch_planes(const BatchPlanesHistParams& p, uint32_t elem_bytes, uint32_t flags, hipStream_t s) {
  if (p.count == 0) return;
  (void)hipMemsetAsync(p.hists, 0, (size_t)elem_bytes * GHF_NSYM * sizeof(uint64_t), s);
  const dim3 grid(p.count < hist_planes_grid(elem_bytes) ? p.count : hist_planes_grid(elem_bytes)), block(kBatchThreads);
  with_elem_bytes(elem_bytes, [&](auto e) { hipLaunchKernelGGL(k_histogram_batch_planes<decltype(e)::value>, grid, block, 0, s, p); });
  launch_histogram_batch_finish(p.hists, elem_bytes, flags, s);
}

void launch_build_codes(const uint64_t* d_hists, uint32_t n_codes, ghf_code* d_codes, int* d_status, uint32_t flags, hipStream_t s) {
  const unsigned long long* const h = reinterpret_cast<const unsigned long long*>(d_hists);
  if (flags & GHF_CODE_LIMIT) hipLaunchKernelGGL(k_build_codes<true>, dim3(n_codes), dim3(64), 0, s, h, d_codes, d_status, flags & GHF_EMPTY_OK);
  else hipLaunchKernelGGL(k_build_codes<false>, dim3(n_codes), dim3(64), 0, s, h, d_codes, d_status, flags & GHF_EMPTY_OK);
}

void launch_batch_planes_raw_auto(const uint64_t* d_hists, const ghf_code* d_codes, uint32_t elem_bytes, uint32_t* d_raw_planes,
                                  hipStream_t s) {
  hipLaunchKernelGGL(k_batch_planes_raw_auto, dim3(1), dim3(kBatchThreads), 0, s, reinterpret_cast<const unsigned long long*>(d_hists),
                     d_codes, elem_bytes, d_raw_planes);
}

// forms: the _forms kernel with raw_planes behind the struct; else the _shared kernel, which takes no mask
void launch_compress_batch_planes(const BatchPlanesCompressParams& p, uint32_t count, uint32_t elem_bytes, bool forms, uint32_t raw_planes,
                                  hipStream_t s) {
  if (count == 0) return;
  const dim3 grid(count * elem_bytes), block(kBatchThreads);
  with_elem_bytes(elem_bytes, [&](auto e) {
    constexpr int E = decltype(e)::value;
    if (forms) hipLaunchKernelGGL(k_compress_batch_planes_forms<E>, grid, block, 0, s, p, raw_planes);
    else hipLaunchKernelGGL(k_compress_batch_planes_shared<E>, grid, block, 0, s, p);
  });
}

void launch_decode_batch_planes(const BatchPlanesDecodeParams& p, uint32_t count, uint32_t elem_bytes, bool forms, uint32_t raw_planes,
                                hipStream_t s) {
  if (count == 0) return;
  const dim3 grid(count), block(kBatchThreads);
  with_elem_bytes(elem_bytes, [&](auto e) {
    constexpr int E = decltype(e)::value;
    if (forms) hipLaunchKernelGGL(k_decode_batch_planes_forms<E>, grid, block, 0, s, p, raw_planes);
    else hipLaunchKernelGGL(k_decode_batch_planes_shared<E>, grid, block, 0, s, p);
  });
}

void launch_decode_bodies_batch_planes(const BatchPlanesBodiesParams& p, uint32_t count, uint32_t elem_bytes, bool forms,
                                       uint32_t raw_planes, hipStream_t s) {
  if (count == 0) return;
  const dim3 grid(count), block(kBatchThreads);
  with_elem_bytes(elem_bytes, [&](auto e) {
    constexpr int E = decltype(e)::value;
    auto write = [&](auto w) {  // p.out_ptrs null: sizes only
      constexpr bool kWrite = decltype(w)::value;
      if (forms) hipLaunchKernelGGL((k_decode_bodies_batch_planes_forms<E, kWrite>), grid, block, 0, s, p, raw_planes);
      else hipLaunchKernelGGL((k_decode_bodies_batch_planes_shared<E, kWrite>), grid, block, 0, s, p);
    };
    if (p.out_ptrs) write(std::true_type());
    else write(std::false_type());
  });
}

}  // namespace ghf
