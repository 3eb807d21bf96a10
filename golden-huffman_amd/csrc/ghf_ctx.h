// golden-huffman_amd/csrc/ghf_ctx.h -- the context behind the C ABI of include/ghf.h.  Host-only and private to the ABI
// units (ghf_api.hip, ghf_api_batch.hip, ghf_api_planes.hip, ghf_api_tensor.hip, ghf_comm.hip): what a ghf_ctx owns on the device, what its
// workspace currently describes, and the few host helpers more than one of those units asks for.
#ifndef GHF_CTX_H_
#define GHF_CTX_H_
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>

#include "ghf_internal.h"

namespace ghf {

// ---- scalars the kernels leave for the host or for each other ------------------------------------------------------
// One copy on the device (ghf_ctx::d) and a pinned mirror of the same type (ghf_ctx::h).  Every member a kernel
// writes is 8 bytes wide, so every device address handed out is 8-byte aligned.

// what one pass of K6 says about itself.  k_sync_pass raises `changed`, counts and takes the maximum in place, so the
// host clears all three with ONE memset in front of every pass: they stay adjacent, in this order.
struct K6Moved {
  uint32_t changed[2];               // [0] some guess moved during the pass; [1] how many did, roughly
  unsigned long long first_inv;      // ~(smallest subsequence whose landing moved); 0: none
};
static_assert(sizeof(K6Moved) == 16 && offsetof(K6Moved, first_inv) == 8, "one 16-byte memset clears flag, count and first");

// what the host reads behind every batch of K6 passes, in ONE copy of sizeof(K6Readback).  The block keeps the 64 bytes
// and the place (24 bytes behind a 256-byte boundary) it has always had: the runtime chooses the kernel that copies it
// by size and alignment, and a block cut to its members, or moved to a 64-byte boundary, is copied by another launch.
struct K6Readback {
  uint64_t n_symbols;  // k_sync_counts: codes in front of the end mark (or in the whole body)
  uint64_t eof_sub;    // first subsequence holding the end mark; nsub: none
  uint64_t unused[3];
  uint64_t landing;    // start[nsub]: bits the last code runs past end_bit (0xFFFF: it ended at an end mark)
  K6Moved moved;       // of the batch's last pass
};
static_assert(sizeof(K6Readback) == 64 && offsetof(K6Readback, moved) % 8 == 0, "one 64-byte copy; 64-bit atomics on moved.first_inv");

struct Scalars {
  uint64_t total_bits;  // K4: body bits of the planned input
  uint64_t end[2];      // K5's d_end: {absolute end bit, bytes} of what ghf_compress / ghf_crs_compress emitted
  K6Readback k6;
  uint64_t start_bit;   // .crs: the body's first bit (k_crs_build_code); ghf_encode_sharded: the shard's, unless the caller keeps it
  // the pinned mirror only: where small reads from device-resident tables land
  int32_t code_lens[2];   // ghf_code::{min_len, max_len}
  uint32_t tree_bytes;    // ghf_tree::tree_bytes
  uint32_t tree_max_len;  // ghf_tree::max_len
};
static_assert(offsetof(Scalars, end) % 8 == 0 && offsetof(Scalars, k6) == 24 && offsetof(Scalars, start_bit) % 8 == 0,
              "8-byte aligned device scalars; the read-back where it has always been");

// ---- buffers that grow on demand ------------------------------------------------------------------------------------
template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;  // in elements
};

template <class T>
void release(DevBuf<T>& b) {
  if (b.p) (void)hipFree(b.p);
  b.p = nullptr;
  b.cap = 0;
}

// ---- what the workspace currently describes ---------------------------------------------------------------------------
// Each cache sits beside the rule that empties it; a forgotten cache describes nothing (`in` / `code` / `stream` null).

// chunk_hist holds K1's per-chunk histograms of (in, n) cut into chunks of `chunk` symbols: K4 need not count again.
// Forgotten when chunk_hist is replaced, and by ghf_histogram_add (a piece's buffer is refilled before anything is planned).
struct HistCache {
  const uint8_t* in = nullptr;
  uint64_t n = 0;
  uint32_t chunk = 0;
  bool describes(const uint8_t* in_, uint64_t n_, uint32_t chunk_) const { return in == in_ && n == n_ && chunk == chunk_; }
  void forget() { in = nullptr; }
};

// chunk_off holds K4's plan of (in, n) under the tables at `code`: what ghf_encode_emit requires.
// Forgotten when chunk_off is replaced and when the tables at `code` are rebuilt.
struct PlanCache {
  const uint8_t* in = nullptr;
  uint64_t n = 0;
  const ghf_code* code = nullptr;
  bool describes(const uint8_t* in_, uint64_t n_, const ghf_code* code_) const { return in == in_ && n == n_ && code == code_; }
  void forget() { in = nullptr; }
};

// d_dt holds the decode tables ghf_decode_prepare built from `code`, for ONE following indexed ghf_decode (the tables
// also hold that decode's work counters).  Forgotten by whatever else writes d_dt and when the tables at `code` are rebuilt.
struct PreparedTables {
  const ghf_code* code = nullptr;
  bool describes(const ghf_code* code_) const { return code == code_; }
  void forget() { code = nullptr; }
};

// fidx is the side-car K6 rebuilt for (stream, bytes), for ONE following decode with index = NULL (the buffer may be
// rewritten afterwards).  Forgotten by every call that is about to rebuild it.
struct RebuiltIndex {
  const uint8_t* stream = nullptr;
  size_t bytes = 0;
  bool describes(const uint8_t* stream_, size_t bytes_) const { return stream == stream_ && bytes == bytes_; }
  void forget() { stream = nullptr; }
};

// ---- THE SLOT RULE (DESIGN.md sections 20 and 23) ----------------------------------------------------------------------------
// A tensor of E = elem_bytes planes is stored in 2 E slots.  Slot p < E is plane p's own: a raw plane lies there as its n_elems
// bytes and has no code, index or table; a dense plane as its .crs2 image of n_elems symbols; a sparse plane as the image of its
// mask, ghf_sparse_mask_bytes(n_elems) symbols.  Slot E + p holds the image of a sparse plane's values, h_n_vals[p] symbols,
// where it has any, and is empty otherwise.  Every driver asks this type which slots hold what; none reads a mask itself.
struct PlaneForms {
  uint32_t elem_bytes;
  unsigned raw_planes, sparse_planes;  // a bit per plane, as asked for (then GHF_*_AUTO may stand in their place) or as chosen
  size_t n_elems;
  const size_t* h_n_vals;  // per plane, where the call has them; read for sparse planes only

  bool is_raw(uint32_t p) const { return ((raw_planes >> p) & 1u) != 0; }
  bool is_sparse(uint32_t p) const { return ((sparse_planes >> p) & 1u) != 0; }
  void store_raw(uint32_t p) { raw_planes |= 1u << p; }
  void store_sparse(uint32_t p) { sparse_planes |= 1u << p; }
  bool all_raw() const { return raw_planes == (1u << elem_bytes) - 1u; }
  size_t mask_bytes() const { return ghf_sparse_mask_bytes(n_elems); }
  // the symbols slot j holds (the bytes, where its plane is raw); 0 behind the planes' own slots: the slot is empty
  size_t symbols(uint32_t j) const {
    const uint32_t p = j % elem_bytes;
    if (j < elem_bytes) return is_sparse(p) ? mask_bytes() : n_elems;
    return is_sparse(p) ? h_n_vals[p] : 0;
  }
  bool stored(uint32_t j) const { return j < elem_bytes || symbols(j) != 0; }
  // ... as a .crs2 image: with a code, and with a side-car or a seek table where the call has them
  bool coded(uint32_t j) const { return stored(j) && !is_raw(j % elem_bytes); }

  // sparse_planes as the compress call (GHF_SPARSE_AUTO alone, or bits below elem_bytes) or the decode (bits only) takes it
  bool sparse_planes_ok(bool may_be_auto) const {
    if (sparse_planes == GHF_SPARSE_AUTO) return may_be_auto;
    return (sparse_planes >> elem_bytes) == 0;
  }
  // raw_planes beside sparse_planes: GHF_RAW_AUTO alone where the call may choose, or bits below elem_bytes; a plane has one
  // form, so where both masks are explicit they share no bit
  bool forms_ok(bool may_be_auto) const {
    if (raw_planes == GHF_RAW_AUTO) return may_be_auto;
    if ((raw_planes >> elem_bytes) != 0) return false;
    return sparse_planes == GHF_SPARSE_AUTO || (raw_planes & sparse_planes) == 0;
  }
};

}  // namespace ghf

struct ghf_ctx {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  int* d_status = nullptr;
  int* h_status = nullptr;  // pinned
  ghf::Scalars* d = nullptr;
  ghf::Scalars* h = nullptr;  // pinned
  uint64_t* d_hist = nullptr;      // [257]
  uint64_t* d_hist_acc = nullptr;  // K1's replicated totals + arrival counter, zero between launches
  ghf_code* d_code = nullptr;      // scratch tables for ghf_compress
  ghf_tree* d_tree = nullptr;      // scratch tree for ghf_crs_compress
  ghf::DecTables* d_dt = nullptr;
  ghf::PreparedTables prepared;
  // encode workspace
  ghf::DevBuf<uint32_t> chunk_hist;  // [chunks][256]
  ghf::HistCache hist;
  ghf::DevBuf<uint64_t> chunk_off;   // [chunks + 1]
  ghf::PlanCache plan;
  ghf::DevBuf<uint64_t> totals;      // per-rank body bits (ghf_encode_sharded)
  // K6 workspace (foreign streams) and the side-car it rebuilds; fidx.d_seg_bit / d_chunk_bit mirror seg_bit.p / chunk_bit.p
  ghf::DevBuf<uint8_t> sync;
  ghf::DevBuf<uint32_t> seg_bit;
  ghf::DevBuf<uint64_t> seg_abs;     // [segments + 1]
  ghf::DevBuf<uint64_t> chunk_bit;
  ghf_index fidx = {};
  ghf::RebuiltIndex rebuilt;
  // ghf_decode_range from a seek table: the side-car of the covered blocks only (describes nothing between calls)
  ghf::DevBuf<uint32_t> range_seg;
  ghf::DevBuf<uint64_t> range_chunk;
  // ghf_decode_planes_range from seek tables: one set of decode tables per plane, alive together for the one expansion
  // launch of all planes and then for each plane's K7 (describes nothing between calls)
  ghf::DevBuf<ghf::DecTables> range_dt;
  // ghf_compress_batch without d_codes: one table set per item (describes nothing between calls)
  ghf::DevBuf<ghf_code> batch_codes;
  // ghf_compress_planes / ghf_decode_planes: elem_bytes byte planes at a stride rounded up to 256 bytes.  Private to the two
  // calls and rewritten by each: what K1 and K4 remember about an address inside it is forgotten before the call returns
  ghf::DevBuf<uint8_t> planes;
  // ghf_histogram_planes / ghf_compress_planes_coded: the 32 replicas k_histogram_planes adds its totals into (zero between
  // launches), and the E x 257 counts of the tensor a ghf_compress_planes_coded is working on (describe nothing between calls).
  // The replicas are zeroed by k_histogram_planes_finish, the launch behind every counting launch: the invariant holds as
  // long as that pair is queued whole.  Where the second launch fails, the host queues a memset of the replicas instead
  // (histogram_planes_into, ghf_api_planes.hip), so that a later histogram on this context does not start from stale sums.
  uint64_t* d_planes_hist_acc = nullptr;
  uint64_t* d_planes_hists = nullptr;  // [GHF_PLANES_MAX][257], and behind them [GHF_PLANES_MAX] image sizes (ghf_compress_planes_forms)
  // ghf_sparse_split / ghf_sparse_merge: the counts of the workgroups' slabs and their exclusive
  // offsets, written and read by the three launches of one call and by nothing else (describe nothing between calls)
  uint64_t* d_sparse_counts = nullptr;  // [kSparseGroups]
  uint64_t* d_sparse_offs = nullptr;    // [kSparseOffWords]
  // ghf_compress_planes_sparse / ghf_decode_planes_sparse: the mask and the values of ONE sparse plane at a time, the mask at
  // [0, mask_stride), the values behind it.  Private to the two calls and refilled for every sparse plane, as `planes` is
  ghf::DevBuf<uint8_t> sparse;
  // ghf_decode_images_batch_stats: where the image decoder counts its rounds and passes (the caller's; null = nowhere)
  uint64_t* images_stats = nullptr;
  // ghf_compress_tensor: what ghf_compress_planes_forms leaves for ghf_tensor_pack -- the 2 E slots, the
  // E rank slots, the 2 E device sizes, and ONE pair of arrays that the side-cars of all stored streams are carved from.
  // Private to the call; they describe nothing between calls and grow on demand
  ghf::DevBuf<uint8_t> tensor_slots;
  ghf::DevBuf<uint8_t> tensor_ranks;
  ghf::DevBuf<uint64_t> tensor_sizes;
  ghf::DevBuf<uint64_t> tensor_chunk_bit;
  ghf::DevBuf<uint32_t> tensor_seg_bit;
  std::string err;
};

namespace ghf {

inline int fail(ghf_ctx* c, int code, const char* what, hipError_t e = hipSuccess) {
  if (c) {
    c->err = what;
    if (e != hipSuccess) {
      c->err += ": ";
      c->err += hipGetErrorString(e);
    }
  }
  return code;
}

#define GHF_HIP(c, call)                                         \
  do {                                                           \
    hipError_t e_ = (call);                                      \
    if (e_ != hipSuccess) return fail((c), GHF_E_HIP, #call, e_); \
  } while (0)

// Makes room for `need` elements: a buffer that is too small is freed and replaced by one of max(need, floor).
// *replaced is set when a new buffer is in place -- whatever described the old one is gone.
template <class T>
int grow(ghf_ctx* c, DevBuf<T>& b, size_t need, size_t floor = 0, bool* replaced = nullptr) {
  if (need <= b.cap) return GHF_OK;
  release(b);
  const size_t cap = std::max(need, floor);
  GHF_HIP(c, hipMalloc(&b.p, cap * sizeof(T)));
  b.cap = cap;
  if (replaced) *replaced = true;
  return GHF_OK;
}

// ---- what more than one of ghf_api.hip, ghf_api_batch.hip and ghf_api_planes.hip ask ------------------------------------
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
// the element widths that have byte-plane kernels
inline bool elem_bytes_ok(uint32_t e) { return e == 2 || e == 4 || e == 8; }

// what a call that queues one launch does around it
template <class Launch>
int queued(ghf_ctx* c, Launch launch) {
  GHF_HIP(c, hipSetDevice(c->device));
  launch();
  GHF_HIP(c, hipGetLastError());
  return GHF_OK;
}

// the part of "this side-car is one of ours" that packing and decoding both ask for
inline bool index_has_arrays(const ghf_index* ix) {
  return ix->d_chunk_bit && ix->d_seg_bit && ix->chunk_symbols == (uint32_t)kBlockSymbols && ix->seg_symbols == (uint32_t)kSegSymbols;
}
// ... and its counts are the ones its n_symbols implies
inline bool index_matches_n(const ghf_index* ix) {
  return index_has_arrays(ix) && ix->n_segs == segs_for(ix->n_symbols) && ix->n_chunks == blocks_for(ix->n_symbols);
}
inline bool index_is_whole(const ghf_index* ix) { return index_matches_n(ix) && ix->n_chunks < kDecMaxGroups; }

// ghf_index and ghf_batch_index: waits for the stream, then frees the two arrays
template <class Index>
int free_index_arrays(ghf_ctx* c, Index* idx) {
  if (!c || !idx) return GHF_E_INVAL;
  GHF_HIP(c, hipSetDevice(c->device));
  GHF_HIP(c, hipStreamSynchronize(c->stream));
  if (idx->d_chunk_bit) (void)hipFree(idx->d_chunk_bit);
  if (idx->d_seg_bit) (void)hipFree(idx->d_seg_bit);
  idx->d_chunk_bit = nullptr;
  idx->d_seg_bit = nullptr;
  return GHF_OK;
}

inline uint32_t le32(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
inline uint64_t le64(const uint8_t* p) { return (uint64_t)le32(p) | ((uint64_t)le32(p + 4) << 32); }

// ---- a range of a seekable stream (defined in ghf_api.hip) -----------------------------------------------------------------
// the part of "this info describes a table of table_bytes" that every consumer of (info, d_table) asks for
int seek_table_ok(ghf_ctx* c, const char* who, const ghf_seek_info* info, const uint8_t* d_table, size_t table_bytes);
// k_seek_expand* for blocks [g0, g1) of one stream's table, under the decode tables at dt (which must be queued first): block g's
// entries land at chunk_bit[g - g0] and seg_bit[(g - g0) * 64]
SeekExpandParams seek_expand_params(ghf_ctx* c, const ghf_seek_info* info, const uint8_t* d_table, const uint8_t* d_stream,
                                    size_t stream_bytes, const DecTables* dt, uint64_t g0, uint64_t g1, uint64_t* chunk_bit,
                                    uint32_t* seg_bit);
// K7 on a view of a side-car that begins at block g -- chunk_bit / seg_bit point at that block's entries -- and ends with
// symbol `end` of a stream of n symbols whose index or seek table carries `index_flags`: a segment's start depends on its own
// block only.  The view's last segment may be cut short by the range; only the stream's own end is followed by the end mark.
// Symbol g * kBlockSymbols lands at out[0]
DecParams range_decode_params(ghf_ctx* c, const uint8_t* d_stream, size_t stream_bytes, DecTables* dt, const uint64_t* chunk_bit,
                              const uint32_t* seg_bit, uint64_t g, uint64_t end, uint64_t n, uint32_t index_flags, uint8_t* out);

// ---- planes in three forms with the context's own side-cars (defined in ghf_api_planes.hip) ---------------------------------------
// ghf_compress_planes_forms under the name `who`.  pooled: the side-cars handed out in h_indexes are views into the context's
// tensor_chunk_bit / tensor_seg_bit, which grow on demand -- nothing is allocated per stream and nothing is the caller's to free;
// they are good until the next pooled call on the context.  Not pooled: ghf_index_alloc per stream, as the public call says
int compress_planes_forms(ghf_ctx* c, const char* who, const uint8_t* d_in, const uint8_t* d_base, size_t n_elems, uint32_t elem_bytes,
                          unsigned raw_planes, unsigned sparse_planes, uint8_t* d_out, size_t slot_bytes, uint64_t* d_out_bytes,
                          ghf_code* d_codes, ghf_index* h_indexes, bool pooled, uint8_t* d_ranks, size_t rank_slot_bytes,
                          unsigned* h_raw_planes, unsigned* h_sparse_planes, size_t* h_n_vals);

}  // namespace ghf
#endif
