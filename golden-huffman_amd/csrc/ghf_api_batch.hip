// golden-huffman_amd/csrc/ghf_api_batch.hip -- the batch family of the C ABI of include/ghf.h (DESIGN.md sections 9, 10, 12,
// 13, 15, 16, 24): many small items in one launch, each under its own code, under one shared code, or as byte planes under one
// code per plane, with the live side-car, from nothing but the bytes, or from stored run records.  Host-side only, like
// ghf_api.hip: argument checks, the parameter block, one launch.  Every step the drivers share -- the message, the rules, the
// fills of a parameter block -- is written once, in front of the drivers that call it.  The ORDER of a driver's checks is part
// of what its caller sees (which of two faults is reported); tests/test_gpu_batch_verdicts.py pins it, and it differs from
// call to call: do not align it in passing.
#include <algorithm>
#include <cstring>
#include <string>

#include "ghf_ctx.h"

using namespace ghf;

namespace {

// ---- the message ------------------------------------------------------------------------------------------------------------
// GHF_E_INVAL with "<entry point>: <what>" for ghf_last_error.  (A plain `return GHF_E_INVAL` leaves the last message alone.)
int refuse(ghf_ctx* c, const char* who, const char* what) { return fail(c, GHF_E_INVAL, (std::string(who) + ": " + what).c_str()); }

// ---- the rules --------------------------------------------------------------------------------------------------------------
constexpr const char* kItemWhat = "max_item_bytes must be 1 .. GHF_BATCH_MAX_ITEM";
constexpr const char* kElemItemWhat = "max_item_bytes must be 1 .. GHF_BATCH_MAX_ITEM and a multiple of elem_bytes";
constexpr const char* kElemWhat = "elem_bytes must be 2, 4 or 8";
constexpr const char* kCapsWhat = "d_out_ptrs without d_out_caps";
constexpr const char* kCodeWhat = "d_code is null or not 16-byte aligned";
constexpr const char* kCodesWhat = "d_codes is null or not 16-byte aligned";
constexpr const char* kMaskWhat = "raw_planes names a plane at or above elem_bytes";

inline bool item_ok(size_t max_item_bytes) { return max_item_bytes != 0 && max_item_bytes <= GHF_BATCH_MAX_ITEM; }
// ... of a batch of elements: a whole number of them
inline bool item_ok(size_t max_item_bytes, uint32_t elem_bytes) { return item_ok(max_item_bytes) && max_item_bytes % elem_bytes == 0; }

// the index covers `count` items of up to max_item_bytes, at the strides the kernels assume
bool batch_index_covers(const ghf_batch_index* ix, uint32_t count, size_t max_item_bytes) {
  return ix->d_chunk_bit && ix->d_seg_bit && ix->count >= count && ix->max_item_bytes >= max_item_bytes && item_ok(ix->max_item_bytes) &&
         ix->blocks_per_item == blocks_for(ix->max_item_bytes) && ix->segs_per_item == segs_for(ix->max_item_bytes);
}
// the slots of count items of elem_bytes planes are counted in 32 bits
inline bool slots_fit(uint32_t count, uint32_t elem_bytes) { return (uint64_t)count * elem_bytes <= 0xFFFFFFFFull; }
// the index covers count * elem_bytes slots of plane_symbols symbols
bool planes_index_covers(const ghf_batch_index* ix, uint32_t count, uint32_t elem_bytes, size_t plane_symbols) {
  return slots_fit(count, elem_bytes) && batch_index_covers(ix, count * elem_bytes, plane_symbols);
}
// a mask of raw planes names planes below elem_bytes only
inline bool mask_ok(uint32_t raw_planes, uint32_t elem_bytes) { return (raw_planes >> elem_bytes) == 0; }
// one code or an array of them: present and where the kernels' 16-byte loads may read it
inline bool code_ok(const ghf_code* d_code) { return d_code && aligned16(d_code); }

// ---- the fills: the member names coincide across the Batch*Params of ghf_internal.h ---------------------------------------------
template <class P>
void fill_in(P& p, const uint8_t* const* d_in_ptrs, const uint64_t* d_in_bytes, size_t max_item_bytes) {
  p.in_ptrs = d_in_ptrs;
  p.in_bytes = d_in_bytes;
  p.max_item_bytes = max_item_bytes;
}
template <class P>
void fill_streams(P& p, const uint8_t* const* d_stream_ptrs, const uint64_t* d_stream_bytes) {
  p.stream_ptrs = d_stream_ptrs;
  p.stream_bytes = d_stream_bytes;
}
template <class P>
void fill_out(P& p, uint8_t* const* d_out_ptrs, const uint64_t* d_out_caps, uint64_t* d_out_bytes, int* d_item_status) {
  p.out_ptrs = d_out_ptrs;
  p.out_caps = d_out_caps;
  p.out_bytes = d_out_bytes;
  p.item_status = d_item_status;
}
// the side-car slices of an index; of none (the compress calls may go without), no side-car is written.  What a slice covers
// goes by three names on the decode side (max_item_bytes, max_plane_symbols, max_slice_symbols): the caller assigns it
template <class P>
void fill_index(P& p, const ghf_batch_index* index) {
  p.chunk_bit = index ? index->d_chunk_bit : nullptr;
  p.seg_bit = index ? index->d_seg_bit : nullptr;
  p.blocks_per_item = index ? index->blocks_per_item : 0;
  p.segs_per_item = index ? index->segs_per_item : 0;
}
// the decoders that find code boundaries and sizes themselves: the largest stream whose bit offsets fit their 32 bits, and
// where ghf_decode_images_batch_stats asked them to count
template <class P>
void fill_bodies(P& p, ghf_ctx* c, size_t max_stream_bytes) {
  p.max_stream_bytes = max_stream_bytes;
  p.stats = c->images_stats;
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------------------------------------- batches
size_t ghf_compress_batch_bound(size_t max_item_bytes) { return ghf_compress_bound(max_item_bytes); }

int ghf_batch_index_alloc(ghf_ctx* c, uint32_t count, size_t max_item_bytes, ghf_batch_index* out) {
  if (!c || !out || !item_ok(max_item_bytes)) return GHF_E_INVAL;
  GHF_HIP(c, hipSetDevice(c->device));
  std::memset(out, 0, sizeof *out);
  out->count = count;
  out->max_item_bytes = max_item_bytes;
  out->blocks_per_item = blocks_for(max_item_bytes);
  out->segs_per_item = segs_for(max_item_bytes);
  GHF_HIP(c, hipMalloc(&out->d_chunk_bit, std::max<size_t>((size_t)count * out->blocks_per_item, 1) * sizeof(uint64_t)));
  hipError_t e = hipMalloc(&out->d_seg_bit, std::max<size_t>((size_t)count * out->segs_per_item, 1) * sizeof(uint32_t));
  if (e != hipSuccess) {
    (void)hipFree(out->d_chunk_bit);
    out->d_chunk_bit = nullptr;
    return fail(c, GHF_E_HIP, "hipMalloc(batch seg_bit)", e);
  }
  return GHF_OK;
}

int ghf_batch_index_free(ghf_ctx* c, ghf_batch_index* idx) { return free_index_arrays(c, idx); }

int ghf_batch_index_item(const ghf_batch_index* idx, uint32_t i, size_t n_i, ghf_index* view) {
  if (!idx || !view || i >= idx->count || n_i > idx->max_item_bytes) return GHF_E_INVAL;
  std::memset(view, 0, sizeof *view);
  index_shape(n_i, view);
  view->d_chunk_bit = idx->d_chunk_bit ? idx->d_chunk_bit + (size_t)i * idx->blocks_per_item : nullptr;
  view->d_seg_bit = idx->d_seg_bit ? idx->d_seg_bit + (size_t)i * idx->segs_per_item : nullptr;
  return GHF_OK;
}

int ghf_compress_batch(ghf_ctx* c, const uint8_t* const* d_in_ptrs, const uint64_t* d_in_bytes, size_t max_item_bytes,
                       uint32_t count, uint8_t* const* d_out_ptrs, const uint64_t* d_out_caps, uint64_t* d_out_bytes,
                       ghf_code* d_codes, const ghf_batch_index* index, int* d_item_status) {
  const char* who = "ghf_compress_batch";
  if (!c) return GHF_E_INVAL;
  if (!item_ok(max_item_bytes)) return refuse(c, who, kItemWhat);
  if (index && !batch_index_covers(index, count, max_item_bytes))
    return refuse(c, who, "index does not cover (count, max_item_bytes) (use ghf_batch_index_alloc)");
  if (count == 0) return GHF_OK;
  if (!d_in_ptrs || !d_in_bytes || !d_out_ptrs || !d_out_caps || !d_out_bytes || !d_item_status) return GHF_E_INVAL;
  GHF_HIP(c, hipSetDevice(c->device));  // in front of the allocation: not `queued`
  if (!d_codes) {
    const int rc = grow(c, c->batch_codes, count);
    if (rc) return rc;
    d_codes = c->batch_codes.p;
  }
  BatchCompressParams p = {};
  fill_in(p, d_in_ptrs, d_in_bytes, max_item_bytes);
  fill_out(p, d_out_ptrs, d_out_caps, d_out_bytes, d_item_status);
  fill_index(p, index);
  p.codes = d_codes;
  launch_compress_batch(p, count, c->stream);
  GHF_HIP(c, hipGetLastError());
  return GHF_OK;
}

int ghf_decode_batch(ghf_ctx* c, const uint8_t* const* d_stream_ptrs, const uint64_t* d_stream_bytes, const ghf_code* d_codes,
                     const ghf_batch_index* index, const uint64_t* d_n_symbols, uint32_t count, uint8_t* const* d_out_ptrs,
                     const uint64_t* d_out_caps, uint64_t* d_out_bytes, int* d_item_status) {
  if (!c || !index) return GHF_E_INVAL;
  if (!batch_index_covers(index, count, 1))
    return refuse(c, "ghf_decode_batch", "index does not cover count items (use ghf_batch_index_alloc)");
  if (count == 0) return GHF_OK;
  if (!d_stream_ptrs || !d_stream_bytes || !d_codes || !d_n_symbols || !d_out_ptrs || !d_out_caps || !d_out_bytes || !d_item_status)
    return GHF_E_INVAL;
  BatchDecodeParams p = {};
  fill_streams(p, d_stream_ptrs, d_stream_bytes);
  fill_out(p, d_out_ptrs, d_out_caps, d_out_bytes, d_item_status);
  fill_index(p, index);
  p.max_item_bytes = index->max_item_bytes;
  p.codes = d_codes;
  p.n_symbols = d_n_symbols;
  return queued(c, [&] { launch_decode_batch(p, count, c->stream); });
}

int ghf_decode_images_batch(ghf_ctx* c, const uint8_t* const* d_stream_ptrs, const uint64_t* d_stream_bytes, uint32_t count,
                            uint8_t* const* d_out_ptrs, const uint64_t* d_out_caps, uint64_t* d_out_bytes, ghf_code* d_codes,
                            int* d_item_status) {
  if (!c || !d_stream_ptrs || !d_stream_bytes || !d_out_bytes || !d_item_status) return GHF_E_INVAL;
  if (d_out_ptrs && !d_out_caps) return refuse(c, "ghf_decode_images_batch", kCapsWhat);
  if (count == 0) return GHF_OK;
  BatchImagesParams p = {};
  fill_streams(p, d_stream_ptrs, d_stream_bytes);
  fill_out(p, d_out_ptrs, d_out_caps, d_out_bytes, d_item_status);
  fill_bodies(p, c, ghf_compress_bound(GHF_BATCH_MAX_ITEM));
  p.codes = d_codes;
  return queued(c, [&] { launch_decode_images_batch(p, count, c->stream); });
}

int ghf_decode_images_batch_stats(ghf_ctx* c, uint64_t* d_stats) {
  if (!c || (reinterpret_cast<uintptr_t>(d_stats) & 7u)) return GHF_E_INVAL;
  c->images_stats = d_stats;
  return GHF_OK;
}

// ---------------------------------------------------------------------------------------------- shared-code batches
int ghf_histogram_batch(ghf_ctx* c, const uint8_t* const* d_in_ptrs, const uint64_t* d_in_bytes, size_t max_item_bytes,
                        uint32_t count, unsigned flags, uint64_t* d_hist) {
  const char* who = "ghf_histogram_batch";
  if (!c) return GHF_E_INVAL;
  if (!item_ok(max_item_bytes)) return refuse(c, who, kItemWhat);
  if (flags & ~GHF_HIST_COVER_ALL) return refuse(c, who, "unknown flags");
  if (!d_in_ptrs || !d_in_bytes || !d_hist) return GHF_E_INVAL;
  if (count == 0) return GHF_OK;
  BatchHistParams p = {};
  fill_in(p, d_in_ptrs, d_in_bytes, max_item_bytes);
  p.count = count;
  p.hist = d_hist;
  return queued(c, [&] { launch_histogram_batch(p, flags, c->stream); });
}

size_t ghf_compress_batch_shared_bound(size_t max_item_bytes) { return (4 * max_item_bytes + 4 + 15) & ~(size_t)15; }

int ghf_compress_batch_shared(ghf_ctx* c, const uint8_t* const* d_in_ptrs, const uint64_t* d_in_bytes, size_t max_item_bytes,
                              uint32_t count, const ghf_code* d_code, uint8_t* const* d_out_ptrs, const uint64_t* d_out_caps,
                              uint64_t* d_out_bytes, const ghf_batch_index* index, int* d_item_status) {
  const char* who = "ghf_compress_batch_shared";
  if (!c) return GHF_E_INVAL;
  if (!item_ok(max_item_bytes)) return refuse(c, who, kItemWhat);
  if (index && !batch_index_covers(index, count, max_item_bytes))
    return refuse(c, who, "index does not cover (count, max_item_bytes) (use ghf_batch_index_alloc)");
  if (!code_ok(d_code)) return refuse(c, who, kCodeWhat);
  if (!d_in_ptrs || !d_in_bytes || !d_out_ptrs || !d_out_caps || !d_out_bytes || !d_item_status) return GHF_E_INVAL;
  if (count == 0) return GHF_OK;
  BatchSharedCompressParams p = {};
  fill_in(p, d_in_ptrs, d_in_bytes, max_item_bytes);
  fill_out(p, d_out_ptrs, d_out_caps, d_out_bytes, d_item_status);
  fill_index(p, index);
  p.code = d_code;
  return queued(c, [&] { launch_compress_batch_shared(p, count, c->stream); });
}

int ghf_decode_batch_shared(ghf_ctx* c, const uint8_t* const* d_stream_ptrs, const uint64_t* d_stream_bytes, const ghf_code* d_code,
                            const ghf_batch_index* index, const uint64_t* d_n_symbols, uint32_t count, uint8_t* const* d_out_ptrs,
                            const uint64_t* d_out_caps, uint64_t* d_out_bytes, int* d_item_status) {
  const char* who = "ghf_decode_batch_shared";
  if (!c || !index) return GHF_E_INVAL;
  if (!batch_index_covers(index, count, 1)) return refuse(c, who, "index does not cover count items (use ghf_batch_index_alloc)");
  if (!code_ok(d_code)) return refuse(c, who, kCodeWhat);
  if (!d_stream_ptrs || !d_stream_bytes || !d_n_symbols || !d_out_ptrs || !d_out_caps || !d_out_bytes || !d_item_status)
    return GHF_E_INVAL;
  if (count == 0) return GHF_OK;
  BatchSharedDecodeParams p = {};
  fill_streams(p, d_stream_ptrs, d_stream_bytes);
  fill_out(p, d_out_ptrs, d_out_caps, d_out_bytes, d_item_status);
  fill_index(p, index);
  p.max_item_bytes = index->max_item_bytes;
  p.code = d_code;
  p.n_symbols = d_n_symbols;
  return queued(c, [&] { launch_decode_batch_shared(p, count, c->stream); });
}

int ghf_decode_bodies_batch_shared(ghf_ctx* c, const uint8_t* const* d_stream_ptrs, const uint64_t* d_stream_bytes,
                                   const ghf_code* d_code, uint32_t count, uint8_t* const* d_out_ptrs, const uint64_t* d_out_caps,
                                   uint64_t* d_out_bytes, int* d_item_status) {
  const char* who = "ghf_decode_bodies_batch_shared";
  if (!c || !d_stream_ptrs || !d_stream_bytes || !d_out_bytes || !d_item_status) return GHF_E_INVAL;
  if (d_out_ptrs && !d_out_caps) return refuse(c, who, kCapsWhat);
  if (!code_ok(d_code)) return refuse(c, who, kCodeWhat);
  if (count == 0) return GHF_OK;
  BatchSharedBodiesParams p = {};
  fill_streams(p, d_stream_ptrs, d_stream_bytes);
  fill_out(p, d_out_ptrs, d_out_caps, d_out_bytes, d_item_status);
  fill_bodies(p, c, ghf_compress_batch_shared_bound(GHF_BATCH_MAX_ITEM));
  p.code = d_code;
  return queued(c, [&] { launch_decode_bodies_batch_shared(p, count, c->stream); });
}

// ---------------------------------------------------------------------------------------------- shared-code batches of byte planes
int ghf_histogram_batch_planes(ghf_ctx* c, const uint8_t* const* d_in_ptrs, const uint64_t* d_in_bytes, size_t max_item_bytes,
                               uint32_t count, uint32_t elem_bytes, unsigned flags, uint64_t* d_hists) {
  const char* who = "ghf_histogram_batch_planes";
  if (!c) return GHF_E_INVAL;
  if (!elem_bytes_ok(elem_bytes)) return refuse(c, who, kElemWhat);
  if (!item_ok(max_item_bytes, elem_bytes)) return refuse(c, who, kElemItemWhat);
  if (flags & ~GHF_HIST_COVER_ALL) return refuse(c, who, "unknown flags");
  if (!d_in_ptrs || !d_in_bytes || !d_hists) return GHF_E_INVAL;
  if (count == 0) return GHF_OK;
  BatchPlanesHistParams p = {};
  fill_in(p, d_in_ptrs, d_in_bytes, max_item_bytes);
  p.count = count;
  p.hists = d_hists;
  return queued(c, [&] { launch_histogram_batch_planes(p, elem_bytes, flags, c->stream); });
}

size_t ghf_compress_batch_planes_shared_bound(size_t max_item_bytes, uint32_t elem_bytes) {
  return elem_bytes_ok(elem_bytes) ? ghf_compress_batch_shared_bound(max_item_bytes / elem_bytes) : 0;
}

// ghf_compress_batch_planes_shared (forms = false: its own kernel, no mask) and ghf_compress_batch_planes_forms
static int compress_batch_planes(ghf_ctx* c, const char* who, bool forms, const uint8_t* const* d_in_ptrs, const uint64_t* d_in_bytes,
                                 size_t max_item_bytes, uint32_t count, uint32_t elem_bytes, const ghf_code* d_codes, uint32_t raw_planes,
                                 uint8_t* const* d_out_ptrs, const uint64_t* d_out_caps, uint64_t* d_out_bytes, const ghf_batch_index* index,
                                 int* d_item_status) {
  if (!c) return GHF_E_INVAL;
  if (!elem_bytes_ok(elem_bytes)) return refuse(c, who, kElemWhat);
  if (!item_ok(max_item_bytes, elem_bytes)) return refuse(c, who, kElemItemWhat);
  if (!slots_fit(count, elem_bytes)) return refuse(c, who, "count * elem_bytes beyond 32 bits");
  if (index && !planes_index_covers(index, count, elem_bytes, max_item_bytes / elem_bytes))
    return refuse(c, who, "index does not cover (count * elem_bytes, max_item_bytes / elem_bytes)");
  if (!code_ok(d_codes)) return refuse(c, who, kCodesWhat);
  if (!mask_ok(raw_planes, elem_bytes)) return refuse(c, who, kMaskWhat);
  if (!d_in_ptrs || !d_in_bytes || !d_out_ptrs || !d_out_caps || !d_out_bytes || !d_item_status) return GHF_E_INVAL;
  if (count == 0) return GHF_OK;
  BatchPlanesCompressParams p = {};
  fill_in(p, d_in_ptrs, d_in_bytes, max_item_bytes);
  fill_out(p, d_out_ptrs, d_out_caps, d_out_bytes, d_item_status);
  fill_index(p, index);
  p.codes = d_codes;
  return queued(c, [&] { launch_compress_batch_planes(p, count, elem_bytes, forms, raw_planes, c->stream); });
}

int ghf_compress_batch_planes_shared(ghf_ctx* c, const uint8_t* const* d_in_ptrs, const uint64_t* d_in_bytes, size_t max_item_bytes,
                                     uint32_t count, uint32_t elem_bytes, const ghf_code* d_codes, uint8_t* const* d_out_ptrs,
                                     const uint64_t* d_out_caps, uint64_t* d_out_bytes, const ghf_batch_index* index,
                                     int* d_item_status) {
  return compress_batch_planes(c, "ghf_compress_batch_planes_shared", false, d_in_ptrs, d_in_bytes, max_item_bytes, count, elem_bytes, d_codes,
                               0, d_out_ptrs, d_out_caps, d_out_bytes, index, d_item_status);
}

int ghf_compress_batch_planes_forms(ghf_ctx* c, const uint8_t* const* d_in_ptrs, const uint64_t* d_in_bytes, size_t max_item_bytes,
                                    uint32_t count, uint32_t elem_bytes, const ghf_code* d_codes, uint32_t raw_planes,
                                    uint8_t* const* d_out_ptrs, const uint64_t* d_out_caps, uint64_t* d_out_bytes,
                                    const ghf_batch_index* index, int* d_item_status) {
  return compress_batch_planes(c, "ghf_compress_batch_planes_forms", true, d_in_ptrs, d_in_bytes, max_item_bytes, count, elem_bytes, d_codes,
                               raw_planes, d_out_ptrs, d_out_caps, d_out_bytes, index, d_item_status);
}

int ghf_batch_planes_raw_auto(ghf_ctx* c, const uint64_t* d_hists, const ghf_code* d_codes, uint32_t elem_bytes, uint32_t* d_raw_planes) {
  const char* who = "ghf_batch_planes_raw_auto";
  if (!c) return GHF_E_INVAL;
  if (!elem_bytes_ok(elem_bytes)) return refuse(c, who, kElemWhat);
  if (!code_ok(d_codes)) return refuse(c, who, kCodesWhat);
  if (!d_hists || !d_raw_planes) return GHF_E_INVAL;
  return queued(c, [&] { launch_batch_planes_raw_auto(d_hists, d_codes, elem_bytes, d_raw_planes, c->stream); });
}

// ghf_decode_batch_planes_shared (forms = false) and ghf_decode_batch_planes_forms
static int decode_batch_planes(ghf_ctx* c, const char* who, bool forms, const uint8_t* const* d_stream_ptrs, const uint64_t* d_stream_bytes,
                               const ghf_code* d_codes, const ghf_batch_index* index, const uint64_t* d_n_elems, uint32_t count,
                               uint32_t elem_bytes, uint32_t raw_planes, uint8_t* const* d_out_ptrs, const uint64_t* d_out_caps,
                               uint64_t* d_out_bytes, int* d_item_status) {
  if (!c || !index) return GHF_E_INVAL;
  if (!elem_bytes_ok(elem_bytes)) return refuse(c, who, kElemWhat);
  if (!planes_index_covers(index, count, elem_bytes, 1)) return refuse(c, who, "index does not cover count * elem_bytes slots");
  if (!code_ok(d_codes)) return refuse(c, who, kCodesWhat);
  if (!mask_ok(raw_planes, elem_bytes)) return refuse(c, who, kMaskWhat);
  if (!d_stream_ptrs || !d_stream_bytes || !d_n_elems || !d_out_ptrs || !d_out_caps || !d_out_bytes || !d_item_status)
    return GHF_E_INVAL;
  if (count == 0) return GHF_OK;
  BatchPlanesDecodeParams p = {};
  fill_streams(p, d_stream_ptrs, d_stream_bytes);
  fill_out(p, d_out_ptrs, d_out_caps, d_out_bytes, d_item_status);
  fill_index(p, index);
  p.max_plane_symbols = index->max_item_bytes;
  p.codes = d_codes;
  p.n_elems = d_n_elems;
  return queued(c, [&] { launch_decode_batch_planes(p, count, elem_bytes, forms, raw_planes, c->stream); });
}

int ghf_decode_batch_planes_shared(ghf_ctx* c, const uint8_t* const* d_stream_ptrs, const uint64_t* d_stream_bytes,
                                   const ghf_code* d_codes, const ghf_batch_index* index, const uint64_t* d_n_elems, uint32_t count,
                                   uint32_t elem_bytes, uint8_t* const* d_out_ptrs, const uint64_t* d_out_caps, uint64_t* d_out_bytes,
                                   int* d_item_status) {
  return decode_batch_planes(c, "ghf_decode_batch_planes_shared", false, d_stream_ptrs, d_stream_bytes, d_codes, index, d_n_elems, count,
                             elem_bytes, 0, d_out_ptrs, d_out_caps, d_out_bytes, d_item_status);
}

int ghf_decode_batch_planes_forms(ghf_ctx* c, const uint8_t* const* d_stream_ptrs, const uint64_t* d_stream_bytes, const ghf_code* d_codes,
                                  const ghf_batch_index* index, const uint64_t* d_n_elems, uint32_t count, uint32_t elem_bytes,
                                  uint32_t raw_planes, uint8_t* const* d_out_ptrs, const uint64_t* d_out_caps, uint64_t* d_out_bytes,
                                  int* d_item_status) {
  return decode_batch_planes(c, "ghf_decode_batch_planes_forms", true, d_stream_ptrs, d_stream_bytes, d_codes, index, d_n_elems, count,
                             elem_bytes, raw_planes, d_out_ptrs, d_out_caps, d_out_bytes, d_item_status);
}

// ghf_decode_bodies_batch_planes_shared (forms = false) and ghf_decode_bodies_batch_planes_forms
static int decode_bodies_batch_planes(ghf_ctx* c, const char* who, bool forms, const uint8_t* const* d_stream_ptrs,
                                      const uint64_t* d_stream_bytes, const ghf_code* d_codes, uint32_t count, uint32_t elem_bytes,
                                      uint32_t raw_planes, uint8_t* const* d_out_ptrs, const uint64_t* d_out_caps, uint64_t* d_out_bytes,
                                      int* d_item_status) {
  if (!c || !d_stream_ptrs || !d_stream_bytes || !d_out_bytes || !d_item_status) return GHF_E_INVAL;
  if (!elem_bytes_ok(elem_bytes)) return refuse(c, who, kElemWhat);
  if (d_out_ptrs && !d_out_caps) return refuse(c, who, kCapsWhat);
  if (!code_ok(d_codes)) return refuse(c, who, kCodesWhat);
  if (!mask_ok(raw_planes, elem_bytes)) return refuse(c, who, kMaskWhat);
  if (count == 0) return GHF_OK;
  BatchPlanesBodiesParams p = {};
  fill_streams(p, d_stream_ptrs, d_stream_bytes);
  fill_out(p, d_out_ptrs, d_out_caps, d_out_bytes, d_item_status);
  fill_bodies(p, c, ghf_compress_batch_shared_bound(GHF_BATCH_MAX_ITEM));
  p.codes = d_codes;
  return queued(c, [&] { launch_decode_bodies_batch_planes(p, count, elem_bytes, forms, raw_planes, c->stream); });
}

int ghf_decode_bodies_batch_planes_shared(ghf_ctx* c, const uint8_t* const* d_stream_ptrs, const uint64_t* d_stream_bytes,
                                          const ghf_code* d_codes, uint32_t count, uint32_t elem_bytes, uint8_t* const* d_out_ptrs,
                                          const uint64_t* d_out_caps, uint64_t* d_out_bytes, int* d_item_status) {
  return decode_bodies_batch_planes(c, "ghf_decode_bodies_batch_planes_shared", false, d_stream_ptrs, d_stream_bytes, d_codes, count, elem_bytes,
                                    0, d_out_ptrs, d_out_caps, d_out_bytes, d_item_status);
}

int ghf_decode_bodies_batch_planes_forms(ghf_ctx* c, const uint8_t* const* d_stream_ptrs, const uint64_t* d_stream_bytes,
                                         const ghf_code* d_codes, uint32_t count, uint32_t elem_bytes, uint32_t raw_planes,
                                         uint8_t* const* d_out_ptrs, const uint64_t* d_out_caps, uint64_t* d_out_bytes, int* d_item_status) {
  return decode_bodies_batch_planes(c, "ghf_decode_bodies_batch_planes_forms", true, d_stream_ptrs, d_stream_bytes, d_codes, count, elem_bytes,
                                    raw_planes, d_out_ptrs, d_out_caps, d_out_bytes, d_item_status);
}

// ---------------------------------------------------------------------------------------------- stored shared-code bodies
size_t ghf_batch_seek_bytes(size_t n_symbols) { return (size_t)batch_seek_bytes_for(n_symbols); }
size_t ghf_batch_seek_bound(size_t max_item_bytes) { return (ghf_batch_seek_bytes(max_item_bytes) + 15) & ~(size_t)15; }

int ghf_batch_seek_pack(ghf_ctx* c, const ghf_batch_index* index, const uint64_t* d_in_bytes, uint32_t count, uint32_t elem_bytes,
                        uint8_t* const* d_rec_ptrs, const uint64_t* d_rec_caps, uint64_t* d_rec_bytes, int* d_slot_status) {
  const char* who = "ghf_batch_seek_pack";
  if (!c || !index) return GHF_E_INVAL;
  if (elem_bytes != 1 && !elem_bytes_ok(elem_bytes)) return refuse(c, who, "elem_bytes must be 1, 2, 4 or 8");
  if (!planes_index_covers(index, count, elem_bytes, 1))
    return refuse(c, who, "index does not cover count * elem_bytes slots (use ghf_batch_index_alloc)");
  if (!d_in_bytes || !d_rec_ptrs || !d_rec_caps || !d_rec_bytes || !d_slot_status) return GHF_E_INVAL;
  if (count == 0) return GHF_OK;
  BatchSeekPackParams p = {};
  fill_index(p, index);
  p.max_slice_symbols = index->max_item_bytes;
  p.in_bytes = d_in_bytes;
  p.elem_bytes = elem_bytes;
  p.rec_ptrs = d_rec_ptrs;
  p.rec_caps = d_rec_caps;
  p.rec_bytes = d_rec_bytes;
  p.slot_status = d_slot_status;
  return queued(c, [&] { launch_batch_seek_pack(p, count * elem_bytes, c->stream); });
}

// the decoders of stored bodies: elem_bytes = 1 is the flat call; the planes calls have vetted elem_bytes themselves, in front
// of the null pointers
static int decode_bodies_batch_seek(ghf_ctx* c, const char* who, const uint8_t* const* d_stream_ptrs, const uint64_t* d_stream_bytes,
                                    const uint8_t* const* d_rec_ptrs, const uint64_t* d_rec_bytes, const ghf_code* d_codes, uint32_t count,
                                    uint32_t elem_bytes, uint8_t* const* d_out_ptrs, const uint64_t* d_out_caps, uint64_t* d_out_bytes,
                                    int* d_item_status, bool forms = false, uint32_t raw_planes = 0) {
  if (!c || !d_stream_ptrs || !d_stream_bytes || !d_rec_ptrs || !d_rec_bytes || !d_out_bytes || !d_item_status) return GHF_E_INVAL;
  if (d_out_ptrs && !d_out_caps) return refuse(c, who, kCapsWhat);
  if (!code_ok(d_codes)) return refuse(c, who, "the code array is null or not 16-byte aligned");
  if (forms && !mask_ok(raw_planes, elem_bytes)) return refuse(c, who, kMaskWhat);
  if (count == 0) return GHF_OK;
  BatchSeekDecodeParams p = {};
  fill_streams(p, d_stream_ptrs, d_stream_bytes);
  fill_out(p, d_out_ptrs, d_out_caps, d_out_bytes, d_item_status);
  p.rec_ptrs = d_rec_ptrs;
  p.rec_bytes = d_rec_bytes;
  p.max_stream_bytes = ghf_compress_batch_shared_bound(GHF_BATCH_MAX_ITEM);
  p.codes = d_codes;
  return queued(c, [&] { launch_decode_bodies_batch_seek(p, count, elem_bytes, forms, raw_planes, c->stream); });
}

int ghf_decode_bodies_batch_shared_seek(ghf_ctx* c, const uint8_t* const* d_stream_ptrs, const uint64_t* d_stream_bytes,
                                        const uint8_t* const* d_rec_ptrs, const uint64_t* d_rec_bytes, const ghf_code* d_code,
                                        uint32_t count, uint8_t* const* d_out_ptrs, const uint64_t* d_out_caps, uint64_t* d_out_bytes,
                                        int* d_item_status) {
  return decode_bodies_batch_seek(c, "ghf_decode_bodies_batch_shared_seek", d_stream_ptrs, d_stream_bytes, d_rec_ptrs, d_rec_bytes, d_code,
                                  count, 1, d_out_ptrs, d_out_caps, d_out_bytes, d_item_status);
}

int ghf_decode_bodies_batch_planes_shared_seek(ghf_ctx* c, const uint8_t* const* d_stream_ptrs, const uint64_t* d_stream_bytes,
                                               const uint8_t* const* d_rec_ptrs, const uint64_t* d_rec_bytes, const ghf_code* d_codes,
                                               uint32_t count, uint32_t elem_bytes, uint8_t* const* d_out_ptrs,
                                               const uint64_t* d_out_caps, uint64_t* d_out_bytes, int* d_item_status) {
  const char* who = "ghf_decode_bodies_batch_planes_shared_seek";
  if (c && !elem_bytes_ok(elem_bytes)) return refuse(c, who, kElemWhat);
  return decode_bodies_batch_seek(c, who, d_stream_ptrs, d_stream_bytes, d_rec_ptrs, d_rec_bytes, d_codes, count, elem_bytes, d_out_ptrs,
                                  d_out_caps, d_out_bytes, d_item_status);
}

int ghf_decode_bodies_batch_planes_forms_seek(ghf_ctx* c, const uint8_t* const* d_stream_ptrs, const uint64_t* d_stream_bytes,
                                              const uint8_t* const* d_rec_ptrs, const uint64_t* d_rec_bytes, const ghf_code* d_codes,
                                              uint32_t count, uint32_t elem_bytes, uint32_t raw_planes, uint8_t* const* d_out_ptrs,
                                              const uint64_t* d_out_caps, uint64_t* d_out_bytes, int* d_item_status) {
  const char* who = "ghf_decode_bodies_batch_planes_forms_seek";
  if (c && !elem_bytes_ok(elem_bytes)) return refuse(c, who, kElemWhat);
  return decode_bodies_batch_seek(c, who, d_stream_ptrs, d_stream_bytes, d_rec_ptrs, d_rec_bytes, d_codes, count, elem_bytes, d_out_ptrs,
                                  d_out_caps, d_out_bytes, d_item_status, true, raw_planes);
}

}  // extern "C"
