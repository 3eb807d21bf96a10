// golden-huffman_amd/csrc/ghf_batch_seek.hip -- stored shared-code bodies: the run record of a body and the decoders that
// follow it (ghf_batch_seek_pack, ghf_decode_bodies_batch_shared_seek, ghf_decode_bodies_batch_planes_shared_seek,
// include/ghf.h; ghf_decode_bodies_batch_planes_forms_seek, where some planes are stored raw:
// section 24).
//
// ghf_decode_batch_shared / ghf_decode_batch_planes_shared follow a live ghf_batch_index: 6.25 % of the input in device
// memory, gone with the process that compressed.  ghf_decode_bodies_batch_shared / .._planes_shared need nothing but the
// bytes and pay for it by finding every code boundary again.  The run record is what a stored batch can keep: the bits
// every run of 128 symbols of ONE body takes, 1.6 % of the input, and the body's decoded size.  A record comes from disk:
// nothing in it is trusted.
#include "ghf_batch_core.h"
#include "ghf_code_rules.h"

namespace ghf {

// ----------------------------------------------------------------------------------------------------------------------
// pack: one workgroup per slot of the index, one lane per run (k_seek_pack's lane per block, at this record's grain).
// Run r is segments 2 r and 2 r + 1 of block r / 32.  The slice is held against what batch_shared_compress_body writes
// before the first store: chunk_bit[0] == 0 (an image of ghf_compress_batch starts behind its header), every block starts
// where its predecessor's last segment ends, segment ends grow, a run fits 16 bits.
// ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBatchThreads) void k_batch_seek_pack(BatchSeekPackParams P) {
  __shared__ int s_bad;
  const int tid = threadIdx.x;
  const uint32_t slot = blockIdx.x;
  auto finish = [&](int status, uint64_t bytes) {  // every lane of the workgroup takes the same exit
    if (tid == 0) {
      P.slot_status[slot] = status;
      P.rec_bytes[slot] = bytes;
    }
  };
  const uint64_t n64 = P.in_bytes[slot / P.elem_bytes];
  uint8_t* const rec = P.rec_ptrs[slot];
  if (n64 == 0) return finish(GHF_E_EMPTY, 0);
  if (n64 % P.elem_bytes || n64 / P.elem_bytes > P.max_slice_symbols || !rec || (reinterpret_cast<uintptr_t>(rec) & 15u))
    return finish(GHF_E_INVAL, 0);
  const uint32_t n = (uint32_t)(n64 / P.elem_bytes);  // <= GHF_BATCH_MAX_ITEM
  const uint32_t bytes = (uint32_t)batch_seek_bytes_for(n);
  if (bytes > P.rec_caps[slot]) return finish(GHF_E_CAP, 0);

  const uint64_t* __restrict__ const chunk_bit = P.chunk_bit + (uint64_t)slot * P.blocks_per_item;
  const uint32_t* __restrict__ const seg_bit = P.seg_bit + (uint64_t)slot * P.segs_per_item;
  const uint32_t nsegs = (uint32_t)segs_for(n), nruns = (uint32_t)batch_runs_for(n);
  if (tid == 0) s_bad = 0;
  __syncthreads();
  // the u16 slots behind the header: the runs, then the padding's zeros
  const uint32_t nslots = (bytes - kBatchSeekHeadBytes) / 2;
  // pass 0 holds the slice against the rules, pass 1 stores: a refused slot writes nothing
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
    for (uint32_t r = tid; r < (pass ? nslots : nruns); r += kBatchThreads) {
      uint32_t bits = 0;
      if (r < nruns) {
        const uint32_t s0 = r * kBatchRunSegs, s1 = s0 + 1 < nsegs ? s0 + 1 : s0;  // the run's segments (the last run may have one)
        const bool first = r % kBatchRunsPerBlock == 0;                            // of its block
        const uint32_t prev = first ? 0u : seg_bit[s0 - 1];
        const uint32_t e0 = seg_bit[s0], e1 = seg_bit[s1];
        bits = e1 - prev;
        if (pass == 0) {
          bool bad = e0 <= prev || (s1 != s0 && e1 <= e0) || bits > 0xFFFFu;
          if (first) {
            const uint32_t b = r / kBatchRunsPerBlock;
            bad |= b == 0 ? chunk_bit[0] != 0 : chunk_bit[b] != chunk_bit[b - 1] + seg_bit[b * (kBlockSymbols / kSegSymbols) - 1];
          }
          if (bad) s_bad = 1;
        }
      }
      if (pass) reinterpret_cast<uint16_t*>(rec + kBatchSeekHeadBytes)[r] = (uint16_t)bits;
    }
    if (pass == 0) {
      __syncthreads();
      if (s_bad) return finish(GHF_E_CORRUPT, 0);  // not the side-car of a body
    }
  }
  if (tid == 0) *reinterpret_cast<uint2*>(rec) = make_uint2(kBatchSeekMagic, n);
  finish(GHF_OK, bytes);
}

// ----------------------------------------------------------------------------------------------------------------------
// a record's header against its size; -> GHF_OK and *n, or GHF_E_FORMAT.  Nothing outside rec[0 .. rec_bytes) is read.
// ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int batch_seek_open(const uint8_t* __restrict__ rec, uint64_t rec_bytes, uint32_t* n) {
  if (rec_bytes < kBatchSeekHeadBytes) return GHF_E_FORMAT;
  const uint2 h = *reinterpret_cast<const uint2*>(rec);
  if (h.x != kBatchSeekMagic || h.y == 0 || h.y > GHF_BATCH_MAX_ITEM || rec_bytes != batch_seek_bytes_for(h.y)) return GHF_E_FORMAT;
  *n = h.y;
  return GHF_OK;
}

struct BatchSeekLds {
  CodeTab t;  // the tables of the code (of the plane) in work
  alignas(16) uint32_t stage[kBatchSeekRoundBytes / 4 + 4];
  uint32_t wave_bits[kBatchWaves];
  CodeVetLds vet;
  int err;
};
static_assert(sizeof(BatchSeekLds) <= 52 * 1024, "three workgroups per CU");

// ----------------------------------------------------------------------------------------------------------------------
// decode, flat items: the front (the code is vetted before the item is looked at), the record's shape, the cap, then the
// rounds of batch_decode_runs (ghf_batch_core.h).  !kWrite: sizes only, the stream is not read.
// ----------------------------------------------------------------------------------------------------------------------
template <bool kWrite>
__global__ __launch_bounds__(kBatchThreads) void k_decode_bodies_batch_shared_seek(BatchSeekDecodeParams P) {
  __shared__ BatchSeekLds S;
  const int tid = threadIdx.x;
  const uint32_t item = blockIdx.x;
  auto finish = [&](int status, uint64_t bytes) {  // every lane of the workgroup takes the same exit
    if (tid == 0) {
      P.item_status[item] = status;
      P.out_bytes[item] = status == GHF_OK ? bytes : 0;
    }
  };
  if (tid == 0) S.err = 0;
  if (!batch_code_ok(S.vet, P.codes, tid)) return finish(GHF_E_FORMAT, 0);

  const uint8_t* const stream = P.stream_ptrs[item];
  const uint8_t* const rec = P.rec_ptrs[item];
  const uint64_t stream_bytes = P.stream_bytes[item];
  uint8_t* const out = kWrite ? P.out_ptrs[item] : nullptr;
  if (!stream || (reinterpret_cast<uintptr_t>(stream) & 15u) || !rec || (reinterpret_cast<uintptr_t>(rec) & 15u) || (kWrite && !out) ||
      stream_bytes > P.max_stream_bytes)
    return finish(GHF_E_INVAL, 0);
  uint32_t n = 0;
  const int shape = batch_seek_open(rec, P.rec_bytes[item], &n);
  if (shape != GHF_OK) return finish(shape, 0);
  if (kWrite) {
    if (n > P.out_caps[item]) return finish(GHF_E_CAP, 0);  // before any store
    int lb, long_from, max_len;
    batch_code_tables(S.t, P.codes, tid, lb, long_from, max_len);
    batch_decode_runs(S, stream, stream_bytes, rec, n, out, lb, long_from, max_len, StoreFlat());
    if (S.err) return finish(GHF_E_CORRUPT, 0);  // (a barrier lies behind the last write of S.err)
  }
  finish(GHF_OK, n);
}

// ----------------------------------------------------------------------------------------------------------------------
// decode, byte planes: one workgroup per ITEM, taking its planes in turn as k_decode_bodies_batch_planes_shared does.  All
// E codes and all E record headers are vetted before the first store; one exit.
// ----------------------------------------------------------------------------------------------------------------------
template <int E, bool kWrite>
__global__ __launch_bounds__(kBatchThreads) void k_decode_bodies_batch_planes_shared_seek(BatchSeekDecodeParams P) {
  __shared__ BatchSeekLds S;
  const int tid = threadIdx.x;
  const uint32_t item = blockIdx.x;
  const size_t slot0 = (size_t)item * E;
  if (tid == 0) S.err = 0;
  int status = GHF_OK;  // the same in every lane, as is all below
#pragma unroll 1
  for (int p = 0; p < E; ++p)
    if (!batch_code_ok(S.vet, P.codes + p, tid)) status = GHF_E_FORMAT;  // (every code is looked at: the barriers stay uniform)
  uint8_t* const out = kWrite && status == GHF_OK ? P.out_ptrs[item] : nullptr;
  uint32_t n = 0;
  if (status == GHF_OK) {
    bool inval = kWrite && !out;
#pragma unroll
    for (int p = 0; p < E; ++p) {
      const uint8_t* const sp = P.stream_ptrs[slot0 + p];
      const uint8_t* const rp = P.rec_ptrs[slot0 + p];
      inval |= !sp || (reinterpret_cast<uintptr_t>(sp) & 15u) || !rp || (reinterpret_cast<uintptr_t>(rp) & 15u) ||
               P.stream_bytes[slot0 + p] > P.max_stream_bytes;
    }
    if (inval) status = GHF_E_INVAL;
  }
  if (status == GHF_OK) {
    bool differ = false;
#pragma unroll 1
    for (int p = 0; p < E && status == GHF_OK; ++p) {
      uint32_t np = 0;
      status = batch_seek_open(P.rec_ptrs[slot0 + p], P.rec_bytes[slot0 + p], &np);
      differ |= p != 0 && np != n;
      n = np;
    }
    if (status == GHF_OK && differ) status = GHF_E_CORRUPT;  // the planes of one item hold the same number of symbols
  }
  if (kWrite) {
    if (status == GHF_OK && (uint64_t)n * E > P.out_caps[item]) status = GHF_E_CAP;  // before any store
#pragma unroll 1
    for (uint32_t p = 0; p < E && status == GHF_OK; ++p) {
      int lb, long_from, max_len;
      batch_code_tables(S.t, P.codes + p, tid, lb, long_from, max_len);
      batch_decode_runs(S, P.stream_ptrs[slot0 + p], P.stream_bytes[slot0 + p], P.rec_ptrs[slot0 + p], n, out, lb, long_from, max_len,
                        StorePlane<E>{p});
      if (S.err) status = GHF_E_CORRUPT;  // (a barrier lies behind the last write of S.err)
    }
  }
  if (tid == 0) {
    P.item_status[item] = status;
    P.out_bytes[item] = status == GHF_OK ? (uint64_t)n * E : 0;
  }
}

// ----------------------------------------------------------------------------------------------------------------------
// decode, byte planes in two forms: bit p of `raw` (a kernel argument, the same in every wave) says
// that plane p is stored as it is.  A raw slot has no record -- its pointer and size are not looked at -- and no code:
// its count is its size, held against its bounds and against the records of the dense planes before the first store.
// (Written out beside its parent: one body for the pair lost timing rows, profiles/batch_planes_bodies/README.md.)
// ----------------------------------------------------------------------------------------------------------------------
template <int E, bool kWrite>
__global__ __launch_bounds__(kBatchThreads) void k_decode_bodies_batch_planes_forms_seek(BatchSeekDecodeParams P, uint32_t raw) {
  __shared__ BatchSeekLds S;
  const int tid = threadIdx.x;
  const uint32_t item = blockIdx.x;
  const size_t slot0 = (size_t)item * E;
  if (tid == 0) S.err = 0;
  int status = GHF_OK;  // the same in every lane, as is all below
#pragma unroll 1
  for (int p = 0; p < E; ++p)
    if (!(raw >> p & 1u) && !batch_code_ok(S.vet, P.codes + p, tid)) status = GHF_E_FORMAT;  // (raw is uniform: so are the barriers)
  __syncthreads();  // (S.err, when every plane is raw)
  uint8_t* const out = kWrite && status == GHF_OK ? P.out_ptrs[item] : nullptr;
  uint32_t n = 0;
  if (status == GHF_OK) {
    bool inval = kWrite && !out;
#pragma unroll
    for (int p = 0; p < E; ++p) {
      const uint8_t* const sp = P.stream_ptrs[slot0 + p];
      inval |= !sp || (reinterpret_cast<uintptr_t>(sp) & 15u);
      if (raw >> p & 1u) {
        inval |= !batch_raw_count_ok<E>(P.stream_bytes[slot0 + p]);
      } else {
        const uint8_t* const rp = P.rec_ptrs[slot0 + p];
        inval |= !rp || (reinterpret_cast<uintptr_t>(rp) & 15u) || P.stream_bytes[slot0 + p] > P.max_stream_bytes;
      }
    }
    if (inval) status = GHF_E_INVAL;
  }
  if (status == GHF_OK) {
    bool differ = false;
#pragma unroll 1
    for (int p = 0; p < E && status == GHF_OK; ++p) {
      uint32_t np = 0;
      if (raw >> p & 1u) np = (uint32_t)P.stream_bytes[slot0 + p];
      else status = batch_seek_open(P.rec_ptrs[slot0 + p], P.rec_bytes[slot0 + p], &np);
      differ |= p != 0 && np != n;
      n = np;
    }
    if (status == GHF_OK && differ) status = GHF_E_CORRUPT;  // the planes of one item hold the same number of symbols
  }
  if (kWrite) {
    if (status == GHF_OK && (uint64_t)n * E > P.out_caps[item]) status = GHF_E_CAP;  // before any store
#pragma unroll 1
    for (uint32_t p = 0; p < E && status == GHF_OK; ++p) {
      if (raw >> p & 1u) {
        batch_raw_plane_copy<E>(S.stage, kBatchSeekRoundBytes, P.stream_ptrs[slot0 + p], n, out, p, tid);
        continue;
      }
      int lb, long_from, max_len;
      batch_code_tables(S.t, P.codes + p, tid, lb, long_from, max_len);
      batch_decode_runs(S, P.stream_ptrs[slot0 + p], P.stream_bytes[slot0 + p], P.rec_ptrs[slot0 + p], n, out, lb, long_from, max_len,
                        StorePlane<E>{p});
      if (S.err) status = GHF_E_CORRUPT;  // (a barrier lies behind the last write of S.err)
    }
  }
  if (tid == 0) {
    P.item_status[item] = status;
    P.out_bytes[item] = status == GHF_OK ? (uint64_t)n * E : 0;
  }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------
void launch_batch_seek_pack(const BatchSeekPackParams& p, uint32_t slots, hipStream_t s) {
  if (slots == 0) return;
  hipLaunchKernelGGL(k_batch_seek_pack, dim3(slots), dim3(kBatchThreads), 0, s, p);
}

// elem_bytes == 1: the flat kernel (no planes, no mask).  Else forms: the _forms_seek kernel with raw_planes behind the
// struct, or the _shared_seek kernel, which takes no mask.  p.out_ptrs null: sizes only
void launch_decode_bodies_batch_seek(const BatchSeekDecodeParams& p, uint32_t count, uint32_t elem_bytes, bool forms, uint32_t raw_planes,
                                     hipStream_t s) {
  if (count == 0) return;
  const dim3 grid(count), block(kBatchThreads);
  if (elem_bytes == 1) {
    if (p.out_ptrs) hipLaunchKernelGGL(k_decode_bodies_batch_shared_seek<true>, grid, block, 0, s, p);
    else hipLaunchKernelGGL(k_decode_bodies_batch_shared_seek<false>, grid, block, 0, s, p);
    return;
  }
  with_elem_bytes(elem_bytes, [&](auto e) {
    constexpr int E = decltype(e)::value;
    auto write = [&](auto w) {
      constexpr bool kWrite = decltype(w)::value;
      if (forms) hipLaunchKernelGGL((k_decode_bodies_batch_planes_forms_seek<E, kWrite>), grid, block, 0, s, p, raw_planes);
      else hipLaunchKernelGGL((k_decode_bodies_batch_planes_shared_seek<E, kWrite>), grid, block, 0, s, p);
    };
    if (p.out_ptrs) write(std::true_type());
    else write(std::false_type());
  });
}

}  // namespace ghf
