// golden-huffman_amd/csrc/ghf_api_planes.hip -- the byte-plane family of the C ABI of include/ghf.h (DESIGN.md sections 14,
// 17 - 21, 23, 25, 26): split / merge / compress, the staged calls, the element range, the calls against a base, sparse planes with
// their rank tables, planes in three forms, and many rows in one call.  Host-side only, like ghf_api.hip: argument checks, workspace, launches.
// Every step the drivers share -- the slot rule, the compress-side checks, the side-cars, packing a dense or a sparse plane,
// decoding a stored stream, the parts of a range -- is written once, in front of the drivers that call it.
#include <algorithm>
#include <cstring>
#include <string>

#include "ghf_ctx.h"

using namespace ghf;

namespace {

inline bool elems_overflow(size_t n_elems, uint32_t e) { return n_elems > (size_t)-1 / e; }
// ... and for the calls that go through the workspace, whose planes sit at n_elems rounded up to 256
inline bool workspace_overflow(size_t n_elems, uint32_t e) { return elems_overflow(n_elems, e) || elems_overflow(n_elems + 255, e); }
inline uint64_t rank_blocks_for(uint64_t n) { return n / kSparseRankElems + (n % kSparseRankElems != 0); }

// The calls against a base share the implementation of their plain calls: a Base says whether the
// call has one, and d_base is null exactly where it has none -- which is what selects the plain kernels in the launchers.
// A delta call with a null or misaligned d_base is refused where the other pointers are.
struct Base {
  bool delta;
  const uint8_t* p;
  bool null() const { return delta && !p; }
  bool misaligned() const { return delta && !aligned16(p); }
};
inline Base no_base() { return {false, nullptr}; }
inline Base base_of(const uint8_t* d_base) { return {true, d_base}; }
// in the family of section 23 d_base is optional: null is the plain call
inline Base base_opt(const uint8_t* d_base) { return d_base ? base_of(d_base) : no_base(); }

// where the ranked compress calls want the rank tables of their sparse planes; the plain calls want none
struct RankOut {
  bool wanted;
  uint8_t* p;
  size_t slot_bytes;
  bool null() const { return wanted && !p; }
  bool misaligned() const { return wanted && (!aligned16(p) || (slot_bytes & 15u)); }
  uint8_t* table(uint32_t plane) const { return wanted ? p + plane * slot_bytes : nullptr; }
};
inline RankOut no_ranks() { return {false, nullptr, 0}; }

// THE SLOT RULE (PlaneForms: which of the 2 E slots hold what) stands in ghf_ctx.h: the container calls of ghf_api_tensor.hip ask it too.

// ---- the workspaces ------------------------------------------------------------------------------------------------------------
// the context's plane workspace for n_elems elements (workspace_overflow has cleared them): *stride <- the distance
// between two planes
int planes_workspace(ghf_ctx* c, size_t n_elems, uint32_t elem_bytes, size_t* stride) {
  *stride = (n_elems + 255) & ~(size_t)255;
  return grow(c, c->planes, *stride * elem_bytes);
}

// the context's second workspace for one sparse plane of n_elems bytes: the mask at [0, *mask_stride), the values behind it
int sparse_workspace(ghf_ctx* c, size_t n_elems, size_t* mask_stride) {
  *mask_stride = (ghf_sparse_mask_bytes(n_elems) + 255) & ~(size_t)255;
  return grow(c, c->sparse, *mask_stride + ((n_elems + 255) & ~(size_t)255));
}

// ---- the steps of the compress drivers -----------------------------------------------------------------------------------------
// What the compress calls check alike behind their null pointers, in this order: elem_bytes; alignment (`aligned_what` names
// what the caller has); the caller's own flags or masks (own() says what is wrong with them, or null); the workspace; the
// side-cars the caller brought; empty; the slots.  A call without a base, codes, ranks or side-cars passes none.
template <class Own>
int compress_args(ghf_ctx* c, const std::string& f, const char* aligned_what, const uint8_t* d_in, Base base, const uint8_t* d_out,
                  size_t slot_bytes, const ghf_code* d_codes, RankOut ranks, size_t n_elems, uint32_t elem_bytes, const ghf_index* indexes,
                  Own own) {
  if (!elem_bytes_ok(elem_bytes)) return fail(c, GHF_E_INVAL, (f + "elem_bytes must be 2, 4 or 8").c_str());
  if (!aligned16(d_in) || !aligned16(d_out) || (slot_bytes & 15u) || !aligned16(d_codes) || base.misaligned())
    return fail(c, GHF_E_INVAL, (f + aligned_what).c_str());
  if (ranks.misaligned()) return fail(c, GHF_E_INVAL, (f + "d_ranks and rank_slot_bytes must be multiples of 16").c_str());
  if (const char* what = own()) return fail(c, GHF_E_INVAL, (f + what).c_str());
  if (workspace_overflow(n_elems, elem_bytes)) return fail(c, GHF_E_INVAL, (f + "n_elems * elem_bytes overflows").c_str());
  for (uint32_t p = 0; indexes && p < elem_bytes; ++p)
    if (indexes[p].n_symbols != n_elems || !index_has_arrays(&indexes[p]))
      return fail(c, GHF_E_INVAL, (f + "an index does not match n_elems (use ghf_index_alloc)").c_str());
  if (n_elems == 0) return fail(c, GHF_E_EMPTY, (f + "no elements").c_str());
  if (slot_bytes < ghf_planes_slot_bytes(n_elems)) return fail(c, GHF_E_CAP, (f + "slot_bytes below ghf_planes_slot_bytes(n_elems)").c_str());
  if (ranks.wanted && ranks.slot_bytes < ghf_sparse_rank_bytes(n_elems))
    return fail(c, GHF_E_CAP, (f + "rank_slot_bytes below ghf_sparse_rank_bytes(n_elems)").c_str());
  return GHF_OK;
}
const char kAlignedPlanes[] = "d_in, d_base, d_out, d_codes and slot_bytes must be multiples of 16";

// k_histogram_planes and its finish on the stream.  The finish is what leaves the replicas zero for the next call: if it
// cannot be queued behind a counting launch that was, a memset takes its place before the error is returned
int histogram_planes_into(ghf_ctx* c, const char* who, const uint8_t* d_in, const uint8_t* d_base, size_t n_elems, uint32_t elem_bytes,
                          unsigned flags, uint64_t* d_hists) {
  const hipError_t e = launch_histogram_planes(d_in, d_base, n_elems, elem_bytes, flags, c->d_planes_hist_acc, d_hists, c->stream);
  if (e == hipSuccess) return GHF_OK;
  (void)hipMemsetAsync(c->d_planes_hist_acc, 0, kPlanesHistAccWords * sizeof(uint64_t), c->stream);
  return fail(c, GHF_E_HIP, who, e);
}

void free_indexes(ghf_ctx* c, ghf_index* ix, uint32_t count) {
  for (uint32_t j = 0; j < count; ++j)
    if (ix[j].d_chunk_bit || ix[j].d_seg_bit) (void)free_index_arrays(c, &ix[j]);
  std::memset(ix, 0, count * sizeof *ix);
}

// the side-cars a compress call hands out (h_indexes may be null: none): one per stream that has a code, of that stream's own
// symbol count; the other entries stay zero.  Nothing is left allocated behind a failure
// pooled (ghf_compress_tensor): the side-cars are views into ONE pair of arrays of the context, which grows on demand
int alloc_sidecars(ghf_ctx* c, const PlaneForms& forms, ghf_index* h_indexes, bool pooled = false) {
  if (!h_indexes) return GHF_OK;
  const uint32_t E = forms.elem_bytes;
  std::memset(h_indexes, 0, 2 * E * sizeof *h_indexes);
  int rc = GHF_OK;
  if (pooled) {
    // every view begins 16-byte aligned: a stream's blocks rounded up to 2 words of 8 bytes, its segments to 4 of 4
    const auto blocks_of = [&](uint32_t j) { return ((size_t)blocks_for(forms.symbols(j)) + 1) & ~(size_t)1; };
    const auto segs_of = [&](uint32_t j) { return ((size_t)segs_for(forms.symbols(j)) + 3) & ~(size_t)3; };
    size_t blocks = 0, segs = 0;
    for (uint32_t j = 0; j < 2 * E; ++j)
      if (forms.coded(j)) blocks += blocks_of(j), segs += segs_of(j);
    if ((rc = grow(c, c->tensor_chunk_bit, std::max<size_t>(blocks, 1)))) return rc;
    if ((rc = grow(c, c->tensor_seg_bit, std::max<size_t>(segs, 1)))) return rc;
    blocks = segs = 0;
    for (uint32_t j = 0; j < 2 * E; ++j) {
      if (!forms.coded(j)) continue;
      index_shape(forms.symbols(j), &h_indexes[j]);
      h_indexes[j].d_chunk_bit = c->tensor_chunk_bit.p + blocks;
      h_indexes[j].d_seg_bit = c->tensor_seg_bit.p + segs;
      blocks += blocks_of(j);
      segs += segs_of(j);
    }
    return GHF_OK;
  }
  for (uint32_t p = 0; p < E && !rc; ++p)
    for (uint32_t j = p; j < 2 * E && !rc; j += E)
      if (forms.coded(j)) rc = ghf_index_alloc(c, forms.symbols(j), &h_indexes[j]);
  if (rc) free_indexes(c, h_indexes, 2 * E);
  return rc;
}

// where a compress call wants slot j: its image, the image's size, its code and its side-car
struct SlotsOut {
  uint8_t* d_out;
  size_t slot_bytes;
  uint64_t* d_out_bytes;
  ghf_code* codes;
  const ghf_index* indexes;  // may be null
  uint8_t* image(uint32_t j) const { return d_out + j * slot_bytes; }
  const ghf_index* index(uint32_t j) const { return indexes ? indexes + j : nullptr; }
};

// compressor.h:70-72 for one plane that stands in the workspace, under a code that is already queued: what ghf_compress_ex does
// behind its code build.  K1 has not seen the plane, so the planner counts it itself (k_chunk_bits_direct)
int pack_dense_plane(ghf_ctx* c, const uint8_t* plane, size_t n_elems, const ghf_code* code, const SlotsOut& out, uint32_t j) {
  int rc;
  if ((rc = ghf_encode_plan(c, plane, n_elems, code, &c->d->total_bits))) return rc;
  if ((rc = ghf_encode_emit(c, plane, n_elems, code, nullptr, GHF_EMIT_LAST | GHF_EMIT_HEADER, out.image(j), out.slot_bytes, out.index(j),
                            c->d->end)))
    return rc;
  launch_store_u64(out.d_out_bytes + j, &c->d->end[1], 0, c->stream);
  GHF_HIP(c, hipGetLastError());
  return GHF_OK;
}

// plane p of E as mask + values, through the second workspace; d_rank_table: where its rank table goes, or null
int pack_sparse_plane(ghf_ctx* c, const uint8_t* plane, size_t n_elems, size_t n_vals, size_t mask_stride, uint8_t* d_rank_table,
                      const SlotsOut& out, uint32_t p, uint32_t E) {
  uint8_t *d_mask = c->sparse.p, *d_vals = c->sparse.p + mask_stride;
  launch_sparse_split(plane, n_elems, d_mask, d_vals, n_elems, c->d_sparse_offs + kSparseOffWords - 1, c->d_sparse_counts, c->d_sparse_offs,
                      c->d_status, c->stream);
  // the plane's rank table, while its mask stands in the workspace; the split is done with the counts and offsets
  if (d_rank_table) launch_sparse_rank_pack(d_mask, n_elems, d_rank_table, c->d_sparse_counts, c->d_sparse_offs, c->d_status, c->stream);
  GHF_HIP(c, hipGetLastError());
  // compressor.h:62-73 for the mask and for the values, each a byte string of its own
  int rc = ghf_compress(c, d_mask, ghf_sparse_mask_bytes(n_elems), out.image(p), out.slot_bytes, out.d_out_bytes + p, out.codes + p, out.index(p));
  if (!rc && n_vals)
    rc = ghf_compress(c, d_vals, n_vals, out.image(E + p), out.slot_bytes, out.d_out_bytes + E + p, out.codes + E + p, out.index(E + p));
  return rc;
}

// ---- the steps of the decode drivers -------------------------------------------------------------------------------------------
// ghf_decode of one stored stream of `symbols` bytes into the workspace at d_to[0 .. cap); `corrupt` is what the caller says of
// a stream of another size
int decode_stored(ghf_ctx* c, const std::string& corrupt, const uint8_t* d_stream, size_t stream_bytes, const ghf_code* d_code,
                  const ghf_index* index, size_t symbols, uint8_t* d_to, size_t cap) {
  int rc;
  if (!index) {  // the side-car-less path: synchronises, and keeps the side-car for the decode that follows
    uint64_t got = 0;
    if ((rc = ghf_decoded_size(c, d_stream, stream_bytes, d_code, &got))) return rc;
    if (got != symbols) return fail(c, GHF_E_CORRUPT, corrupt.c_str());
  }
  return ghf_decode(c, d_stream, stream_bytes, d_code, index, d_to, cap, nullptr);
}

// the caller's arrays of a range call, an entry per slot: either indexes, or the three arrays of the seek tables
struct StoredStreams {
  const uint8_t* const* ptrs;
  const size_t* bytes;
  const ghf_code* d_codes;
  const ghf_index* indexes;
  const ghf_seek_info* h_infos;
  const uint8_t* const* h_table_ptrs;
  const size_t* h_table_bytes;
  bool by_table() const { return h_infos || h_table_ptrs || h_table_bytes; }
  bool one_source() const { return (indexes != nullptr) != by_table() && (!by_table() || (h_infos && h_table_ptrs && h_table_bytes)); }
  uint64_t symbols(uint32_t j) const { return by_table() ? h_infos[j].n_symbols : indexes[j].n_symbols; }
  bool index_ok(uint32_t j) const { return by_table() || indexes[j].n_symbols == 0 || index_is_whole(&indexes[j]); }
};

// one stored stream of a range call: which symbols of it the call decodes, and where to
struct RangePart {
  uint32_t slot;      // in the caller's arrays
  uint64_t lo, hi;    // symbols [lo, hi) of the stream; lo is a multiple of kBlockSymbols
  uint64_t symbols;   // of the whole stream
  uint8_t* to;        // symbol lo lands here (16-byte aligned)
  size_t cap;
};

// Every part into its place, and behind(slot) queued behind each.  From side-cars that is ghf_decode_range per part.  From seek
// tables ghf_decode_range would expand every stream by itself, and k_seek_expand has a latency floor -- a lane walks its 512
// symbols serially -- that a range does not shrink: the floors one after the other cost more than decoding the whole tensor from
// side-cars (DESIGN.md section 17 has the measurement).  So: expand(x, n_parts) queues the decode tables of slot j at range_dt[j]
// (n_dt of them, alive until the slot's K7 has run) and then ONE launch that expands the covered blocks of all parts; K7 follows
// per part on that view, set up as ghf_decode_range sets it up (a part begins on a block, so there is no head).
template <class Expand, class Behind>
int decode_parts(ghf_ctx* c, const StoredStreams& s, const RangePart* parts, uint32_t n_parts, size_t n_dt, Expand expand, Behind behind) {
  int rc;
  if (!s.by_table()) {
    for (uint32_t i = 0; i < n_parts; ++i) {
      const uint32_t j = parts[i].slot;
      if ((rc = ghf_decode_range(c, s.ptrs[j], s.bytes[j], s.d_codes + j, s.indexes + j, nullptr, nullptr, 0, parts[i].lo,
                                 parts[i].hi - parts[i].lo, parts[i].to, parts[i].cap)))
        return rc;
      behind(j);
    }
    return GHF_OK;
  }
  const size_t segs_per_block = kBlockSymbols / kSegSymbols;
  size_t blocks = 0;
  for (uint32_t i = 0; i < n_parts; ++i) blocks += (size_t)(blocks_for(parts[i].hi) - parts[i].lo / kBlockSymbols);
  if (!(rc = grow(c, c->range_dt, n_dt))) rc = grow(c, c->range_chunk, blocks, 1024);
  if (!rc) rc = grow(c, c->range_seg, blocks * segs_per_block, 1024 * 64);
  if (rc) return rc;
  SeekExpandParams x[kSeekStreamsMax];
  size_t at = 0;
  for (uint32_t i = 0; i < n_parts; ++i) {
    const uint32_t j = parts[i].slot;
    x[i] = seek_expand_params(c, s.h_infos + j, s.h_table_ptrs[j], s.ptrs[j], s.bytes[j], c->range_dt.p + j, parts[i].lo / kBlockSymbols,
                              blocks_for(parts[i].hi), c->range_chunk.p + at, c->range_seg.p + at * segs_per_block);
    at += (size_t)(x[i].g1 - x[i].g0);
  }
  if ((rc = expand(x, n_parts))) return rc;
  for (uint32_t i = 0; i < n_parts; ++i) {
    const uint32_t j = parts[i].slot;
    launch_decode(range_decode_params(c, s.ptrs[j], s.bytes[j], c->range_dt.p + j, x[i].chunk_bit, x[i].seg_bit, x[i].g0, parts[i].hi,
                                      parts[i].symbols, s.h_infos[j].flags, parts[i].to),
                  c->stream);
    behind(j);
  }
  return GHF_OK;
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------------------------------------- byte planes
// (no reference counterpart)
size_t ghf_planes_slot_bytes(size_t n_elems) { return (ghf_compress_bound(n_elems) + 15) & ~(size_t)15; }

// what ghf_planes_split and ghf_planes_merge check alike: `d_inter` is the interleaved side
static int planes_args(ghf_ctx* c, const char* who, const uint8_t* d_inter, const uint8_t* d_planes, size_t plane_stride, size_t n_elems,
                       uint32_t elem_bytes, Base base) {
  if (!c || !d_inter || !d_planes || base.null()) return GHF_E_INVAL;
  const std::string f = std::string(who) + ": ";
  if (!elem_bytes_ok(elem_bytes)) return fail(c, GHF_E_INVAL, (f + "elem_bytes must be 2, 4 or 8").c_str());
  if (!aligned16(d_inter) || !aligned16(d_planes) || (plane_stride & 15u) || base.misaligned())
    return fail(c, GHF_E_INVAL, (f + "pointers and plane_stride must be multiples of 16").c_str());
  if (elems_overflow(n_elems, elem_bytes)) return fail(c, GHF_E_INVAL, (f + "n_elems * elem_bytes overflows").c_str());
  if (n_elems == 0) return fail(c, GHF_E_EMPTY, (f + "no elements").c_str());
  if (plane_stride < n_elems) return fail(c, GHF_E_CAP, (f + "plane_stride below n_elems").c_str());
  return GHF_OK;
}

static int planes_split(ghf_ctx* c, const char* who, const uint8_t* d_in, Base base, size_t n_elems, uint32_t elem_bytes,
                        uint8_t* d_planes, size_t plane_stride) {
  const int rc = planes_args(c, who, d_in, d_planes, plane_stride, n_elems, elem_bytes, base);
  if (rc) return rc;
  return queued(c, [&] { launch_planes_split(d_in, base.p, n_elems, elem_bytes, d_planes, plane_stride, c->stream); });
}
int ghf_planes_split(ghf_ctx* c, const uint8_t* d_in, size_t n_elems, uint32_t elem_bytes, uint8_t* d_planes, size_t plane_stride) {
  return planes_split(c, "ghf_planes_split", d_in, no_base(), n_elems, elem_bytes, d_planes, plane_stride);
}

static int planes_merge(ghf_ctx* c, const char* who, const uint8_t* d_planes, size_t plane_stride, Base base, size_t n_elems,
                        uint32_t elem_bytes, uint8_t* d_out) {
  const int rc = planes_args(c, who, d_out, d_planes, plane_stride, n_elems, elem_bytes, base);
  if (rc) return rc;
  return queued(c, [&] { launch_planes_merge(d_planes, plane_stride, base.p, n_elems, elem_bytes, d_out, nullptr, c->stream); });
}
int ghf_planes_merge(ghf_ctx* c, const uint8_t* d_planes, size_t plane_stride, size_t n_elems, uint32_t elem_bytes, uint8_t* d_out) {
  return planes_merge(c, "ghf_planes_merge", d_planes, plane_stride, no_base(), n_elems, elem_bytes, d_out);
}

static int planes_merge_range(ghf_ctx* c, const char* who, const uint8_t* d_planes, size_t plane_stride, Base base, size_t first,
                              size_t count, uint32_t elem_bytes, uint8_t* d_out) {
  const std::string f = std::string(who) + ": ";
  if (c && first + count < first) return fail(c, GHF_E_INVAL, (f + "first + count overflows").c_str());
  int rc = planes_args(c, who, d_out, d_planes, plane_stride, count, elem_bytes, base);
  if (!rc && plane_stride < first + count) rc = fail(c, GHF_E_CAP, (f + "plane_stride below first + count").c_str());
  if (rc) return rc;
  return queued(c, [&] { launch_planes_merge_range(d_planes, plane_stride, base.p, first, count, elem_bytes, d_out, nullptr, c->stream); });
}
int ghf_planes_merge_range(ghf_ctx* c, const uint8_t* d_planes, size_t plane_stride, size_t first, size_t count, uint32_t elem_bytes,
                           uint8_t* d_out) {
  return planes_merge_range(c, "ghf_planes_merge_range", d_planes, plane_stride, no_base(), first, count, elem_bytes, d_out);
}

int ghf_compress_planes(ghf_ctx* c, const uint8_t* d_in, size_t n_elems, uint32_t elem_bytes, uint8_t* d_out, size_t slot_bytes,
                        uint64_t* d_out_bytes, ghf_code* d_codes, const ghf_index* indexes) {
  if (!c || !d_in || !d_out || !d_out_bytes) return GHF_E_INVAL;
  // d_codes is optional here and goes to ghf_compress plane by plane: its alignment is not this call's to ask
  int rc = compress_args(c, "ghf_compress_planes: ", "d_in, d_out and slot_bytes must be multiples of 16", d_in, no_base(), d_out, slot_bytes,
                         nullptr, no_ranks(), n_elems, elem_bytes, indexes, [] { return (const char*)nullptr; });
  if (rc) return rc;
  GHF_HIP(c, hipSetDevice(c->device));
  size_t stride = 0;
  if ((rc = planes_workspace(c, n_elems, elem_bytes, &stride))) return rc;
  launch_planes_split(d_in, nullptr, n_elems, elem_bytes, c->planes.p, stride, c->stream);
  GHF_HIP(c, hipGetLastError());
  for (uint32_t p = 0; p < elem_bytes && !rc; ++p)  // compressor.h:62-73, once per plane
    rc = ghf_compress(c, c->planes.p + p * stride, n_elems, d_out + p * slot_bytes, slot_bytes, d_out_bytes + p,
                      d_codes ? d_codes + p : nullptr, indexes ? indexes + p : nullptr);
  // the workspace is private and the next call refills the same addresses with other bytes
  c->hist.forget();
  c->plan.forget();
  return rc;
}

// ---------------------------------------------------------------------------------------------- byte planes in stages
// (no reference counterpart)
static int histogram_planes(ghf_ctx* c, const char* who, const uint8_t* d_in, Base base, size_t n_elems, uint32_t elem_bytes,
                            unsigned flags, uint64_t* d_hists) {
  if (!c || !d_in || !d_hists || base.null()) return GHF_E_INVAL;
  const std::string f = std::string(who) + ": ";
  if (!elem_bytes_ok(elem_bytes)) return fail(c, GHF_E_INVAL, (f + "elem_bytes must be 2, 4 or 8").c_str());
  if (!aligned16(d_in) || base.misaligned()) return fail(c, GHF_E_INVAL, (f + "d_in and d_base must be 16-byte aligned").c_str());
  if (flags & ~GHF_HIST_COVER_ALL) return fail(c, GHF_E_INVAL, (f + "unknown flags").c_str());
  if (elems_overflow(n_elems, elem_bytes)) return fail(c, GHF_E_INVAL, (f + "n_elems * elem_bytes overflows").c_str());
  if (n_elems == 0) return fail(c, GHF_E_EMPTY, (f + "no elements").c_str());
  GHF_HIP(c, hipSetDevice(c->device));
  return histogram_planes_into(c, (f + "launch").c_str(), d_in, base.p, n_elems, elem_bytes, flags, d_hists);
}
int ghf_histogram_planes(ghf_ctx* c, const uint8_t* d_in, size_t n_elems, uint32_t elem_bytes, unsigned flags, uint64_t* d_hists) {
  return histogram_planes(c, "ghf_histogram_planes", d_in, no_base(), n_elems, elem_bytes, flags, d_hists);
}

int ghf_planes_image_bytes(ghf_ctx* c, const uint64_t* d_hists, const ghf_code* d_codes, uint32_t elem_bytes, uint64_t* d_bytes) {
  if (!c || !d_hists || !d_codes || !d_bytes) return GHF_E_INVAL;
  if (!elem_bytes_ok(elem_bytes)) return fail(c, GHF_E_INVAL, "ghf_planes_image_bytes: elem_bytes must be 2, 4 or 8");
  return queued(c, [&] { launch_planes_image_bytes(d_hists, d_codes, elem_bytes, d_bytes, c->stream); });
}

static int compress_planes_coded(ghf_ctx* c, const char* who, const uint8_t* d_in, Base base, size_t n_elems, uint32_t elem_bytes,
                                 ghf_code* d_codes, unsigned flags, uint8_t* d_out, size_t slot_bytes, uint64_t* d_out_bytes,
                                 const ghf_index* indexes) {
  if (!c || !d_in || !d_out || !d_out_bytes || !d_codes || base.null()) return GHF_E_INVAL;
  const std::string f = std::string(who) + ": ";
  int rc = compress_args(c, f, kAlignedPlanes, d_in, base, d_out, slot_bytes, d_codes, no_ranks(), n_elems, elem_bytes, indexes,
                         [&] { return (flags & ~GHF_PLANES_BUILD_CODES) ? "unknown flags" : nullptr; });
  if (rc) return rc;
  GHF_HIP(c, hipSetDevice(c->device));
  size_t stride = 0;
  if ((rc = planes_workspace(c, n_elems, elem_bytes, &stride))) return rc;
  // compressor.h:63 for all planes in one pass over the interleaved buffer, then compressor.h:64 for all planes in one launch --
  // or the caller's codes, held against the counts
  if ((rc = histogram_planes_into(c, (f + "histogram launch").c_str(), d_in, base.p, n_elems, elem_bytes, 0, c->d_planes_hists))) return rc;
  if (flags & GHF_PLANES_BUILD_CODES) {
    if ((rc = ghf_build_codes(c, c->d_planes_hists, elem_bytes, d_codes, 0))) return rc;
  } else {
    launch_planes_vet_codes(c->d_planes_hists, d_codes, elem_bytes, c->d_status, c->stream);
    GHF_HIP(c, hipGetLastError());
  }
  launch_planes_split(d_in, base.p, n_elems, elem_bytes, c->planes.p, stride, c->stream);
  GHF_HIP(c, hipGetLastError());
  // K1 has not seen these planes: whatever it remembers about an address inside the workspace is of another call
  c->hist.forget();
  const SlotsOut out = {d_out, slot_bytes, d_out_bytes, d_codes, indexes};
  for (uint32_t p = 0; p < elem_bytes && !rc; ++p) rc = pack_dense_plane(c, c->planes.p + p * stride, n_elems, d_codes + p, out, p);
  c->hist.forget();
  c->plan.forget();
  return rc;
}
int ghf_compress_planes_coded(ghf_ctx* c, const uint8_t* d_in, size_t n_elems, uint32_t elem_bytes, ghf_code* d_codes, unsigned flags,
                              uint8_t* d_out, size_t slot_bytes, uint64_t* d_out_bytes, const ghf_index* indexes) {
  return compress_planes_coded(c, "ghf_compress_planes_coded", d_in, no_base(), n_elems, elem_bytes, d_codes, flags, d_out, slot_bytes,
                               d_out_bytes, indexes);
}

static int decode_planes(ghf_ctx* c, const char* who, const uint8_t* const* h_stream_ptrs, const size_t* h_stream_bytes,
                         const ghf_code* d_codes, const ghf_index* indexes, Base base, size_t n_elems, uint32_t elem_bytes, uint8_t* d_out,
                         size_t cap, uint64_t* d_out_bytes) {
  if (!c || !h_stream_ptrs || !h_stream_bytes || !d_codes || !d_out || base.null()) return GHF_E_INVAL;
  const std::string f = std::string(who) + ": ";
  if (!elem_bytes_ok(elem_bytes)) return fail(c, GHF_E_INVAL, (f + "elem_bytes must be 2, 4 or 8").c_str());
  for (uint32_t p = 0; p < elem_bytes; ++p)
    if (!h_stream_ptrs[p] || !aligned16(h_stream_ptrs[p])) return fail(c, GHF_E_INVAL, (f + "a stream pointer is null or not 16-byte aligned").c_str());
  if (!aligned16(d_out) || base.misaligned()) return fail(c, GHF_E_INVAL, (f + "d_out and d_base must be 16-byte aligned").c_str());
  if (workspace_overflow(n_elems, elem_bytes)) return fail(c, GHF_E_INVAL, (f + "n_elems * elem_bytes overflows").c_str());
  for (uint32_t p = 0; indexes && p < elem_bytes; ++p)
    if (indexes[p].n_symbols != n_elems || !index_is_whole(&indexes[p]))
      return fail(c, GHF_E_INVAL, (f + "an index does not cover exactly n_elems symbols").c_str());
  if (n_elems == 0) return fail(c, GHF_E_EMPTY, (f + "no elements").c_str());
  if (cap < n_elems * elem_bytes) return fail(c, GHF_E_CAP, (f + "output capacity below n_elems * elem_bytes").c_str());
  GHF_HIP(c, hipSetDevice(c->device));
  size_t stride = 0;
  int rc = planes_workspace(c, n_elems, elem_bytes, &stride);
  if (rc) return rc;
  for (uint32_t p = 0; p < elem_bytes; ++p)
    if ((rc = decode_stored(c, f + "a plane does not decode to n_elems bytes", h_stream_ptrs[p], h_stream_bytes[p], d_codes + p,
                            indexes ? indexes + p : nullptr, n_elems, c->planes.p + p * stride, stride)))
      return rc;
  launch_planes_merge(c->planes.p, stride, base.p, n_elems, elem_bytes, d_out, c->d_status, c->stream);  // nothing is stored behind a failed decode
  if (d_out_bytes) launch_store_u64(d_out_bytes, nullptr, (uint64_t)n_elems * elem_bytes, c->stream);
  GHF_HIP(c, hipGetLastError());
  return GHF_OK;
}
int ghf_decode_planes(ghf_ctx* c, const uint8_t* const* h_stream_ptrs, const size_t* h_stream_bytes, const ghf_code* d_codes,
                      const ghf_index* indexes, size_t n_elems, uint32_t elem_bytes, uint8_t* d_out, size_t cap, uint64_t* d_out_bytes) {
  return decode_planes(c, "ghf_decode_planes", h_stream_ptrs, h_stream_bytes, d_codes, indexes, no_base(), n_elems, elem_bytes, d_out, cap,
                       d_out_bytes);
}

// ---------------------------------------------------------------------------------------------- element range of byte planes
// (no reference counterpart)
// what the range asks of its arguments; GHF_OK: the work below may be queued, unless count == 0
static int decode_planes_range_checks(ghf_ctx* c, const char* who, const StoredStreams& s, Base base, uint32_t elem_bytes, uint64_t first,
                                      uint64_t count, const uint8_t* d_out, size_t cap) {
  if (!c || !s.ptrs || !s.bytes || !s.d_codes || !d_out || base.null()) return GHF_E_INVAL;
  const std::string f = std::string(who) + ": ";
  if (!elem_bytes_ok(elem_bytes)) return fail(c, GHF_E_INVAL, (f + "elem_bytes must be 2, 4 or 8").c_str());
  if (!s.one_source())
    return fail(c, GHF_E_INVAL, (f + "exactly one of indexes / (h_infos, h_table_ptrs, h_table_bytes) must be given").c_str());
  const bool by_table = s.by_table();
  for (uint32_t p = 0; p < elem_bytes; ++p) {
    if (!s.ptrs[p] || !aligned16(s.ptrs[p])) return fail(c, GHF_E_INVAL, (f + "a stream pointer is null or not 16-byte aligned").c_str());
    if (by_table && (!s.h_table_ptrs[p] || !aligned16(s.h_table_ptrs[p])))
      return fail(c, GHF_E_INVAL, (f + "a table pointer is null or not 16-byte aligned").c_str());
  }
  if (!aligned16(d_out) || base.misaligned()) return fail(c, GHF_E_INVAL, (f + "d_out and d_base must be 16-byte aligned").c_str());
  const uint64_t n_elems = s.symbols(0);
  for (uint32_t p = 0; p < elem_bytes; ++p) {
    if (!s.index_ok(p)) return fail(c, GHF_E_INVAL, (f + "malformed index").c_str());
    if (s.symbols(p) != n_elems) return fail(c, GHF_E_INVAL, (f + "the planes disagree on n_symbols").c_str());
  }
  if (first > n_elems || count > n_elems - first) return fail(c, GHF_E_INVAL, (f + "first + count exceeds n_elems").c_str());
  // the workspace holds the range from the start of its first block (below), and a vector more for the merge's second load
  const size_t lead = (size_t)(first % kBlockSymbols);
  if (count > (size_t)-1 - lead - 16 || workspace_overflow((size_t)count + lead + 16, elem_bytes))
    return fail(c, GHF_E_INVAL, (f + "count * elem_bytes overflows").c_str());
  for (uint32_t p = 0; by_table && p < elem_bytes; ++p) {  // every plane before anything is queued for the first
    const int rc = seek_table_ok(c, who, s.h_infos + p, s.h_table_ptrs[p], s.h_table_bytes[p]);
    if (rc) return rc;
  }
  if (cap < count * elem_bytes) return fail(c, GHF_E_CAP, (f + "output capacity below count * elem_bytes").c_str());
  return GHF_OK;
}

// elements [first, first + count), count != 0, of planes that passed the checks above
static int decode_planes_range_work(ghf_ctx* c, const StoredStreams& s, Base base, uint32_t elem_bytes, uint64_t first, uint64_t count,
                                    uint8_t* d_out) {
  GHF_HIP(c, hipSetDevice(c->device));
  // Every plane is decoded from the start of the block that holds `first`: plane p's byte `first - lead` lands on the
  // 16-byte aligned start of its workspace plane, so every later byte sits at an address congruent to its index modulo 16 --
  // what K7's 16-byte store path asks for -- and no block is entered in its middle: ghf_decode_range queues no k_decode_head,
  // whose one wave walks up to a block serially (DESIGN.md section 17 has the measurement).  The up to 4095 symbols in front
  // of the range are one K7 block of work; the merge skips them and takes the skew out.
  const size_t lead = (size_t)(first % kBlockSymbols);
  size_t stride = 0;
  int rc = planes_workspace(c, (size_t)count + lead + 16, elem_bytes, &stride);
  if (rc) return rc;
  RangePart parts[GHF_PLANES_MAX];
  for (uint32_t p = 0; p < elem_bytes; ++p) parts[p] = {p, first - lead, first + count, s.symbols(p), c->planes.p + p * stride, stride};
  // from tables: all E table sets first, then the one expansion of all planes (k_seek_expand_planes)
  const auto expand = [&](const SeekExpandParams* x, uint32_t n) {
    SeekExpandPlanesParams a = {};
    std::copy(x, x + n, a.plane);
    for (uint32_t p = 0; p < n; ++p) launch_build_decode_tables(s.d_codes + p, c->range_dt.p + p, c->d_status, c->stream);
    launch_seek_expand_planes(a, n, c->stream);
    return (int)GHF_OK;
  };
  if ((rc = decode_parts(c, s, parts, elem_bytes, elem_bytes, expand, [](uint32_t) {}))) return rc;
  launch_planes_merge_range(c->planes.p, stride, base.p, lead, count, elem_bytes, d_out, c->d_status, c->stream);  // nothing behind a failed decode
  GHF_HIP(c, hipGetLastError());
  return GHF_OK;
}

static int decode_planes_range(ghf_ctx* c, const char* who, const uint8_t* const* h_stream_ptrs, const size_t* h_stream_bytes,
                               const ghf_code* d_codes, const ghf_index* indexes, const ghf_seek_info* h_infos,
                               const uint8_t* const* h_table_ptrs, const size_t* h_table_bytes, Base base, uint32_t elem_bytes,
                               uint64_t first, uint64_t count, uint8_t* d_out, size_t cap) {
  const StoredStreams s = {h_stream_ptrs, h_stream_bytes, d_codes, indexes, h_infos, h_table_ptrs, h_table_bytes};
  const int rc = decode_planes_range_checks(c, who, s, base, elem_bytes, first, count, d_out, cap);
  if (rc || count == 0) return rc;
  return decode_planes_range_work(c, s, base, elem_bytes, first, count, d_out);
}
int ghf_decode_planes_range(ghf_ctx* c, const uint8_t* const* h_stream_ptrs, const size_t* h_stream_bytes, const ghf_code* d_codes,
                            const ghf_index* indexes, const ghf_seek_info* h_infos, const uint8_t* const* h_table_ptrs,
                            const size_t* h_table_bytes, uint32_t elem_bytes, uint64_t first, uint64_t count, uint8_t* d_out, size_t cap) {
  return decode_planes_range(c, "ghf_decode_planes_range", h_stream_ptrs, h_stream_bytes, d_codes, indexes, h_infos, h_table_ptrs,
                             h_table_bytes, no_base(), elem_bytes, first, count, d_out, cap);
}

// ---------------------------------------------------------------------------------------------- byte planes against a base
// (no reference counterpart): the calls above with the XOR against d_base in their streaming kernels
int ghf_histogram_planes_delta(ghf_ctx* c, const uint8_t* d_in, const uint8_t* d_base, size_t n_elems, uint32_t elem_bytes, unsigned flags,
                               uint64_t* d_hists) {
  return histogram_planes(c, "ghf_histogram_planes_delta", d_in, base_of(d_base), n_elems, elem_bytes, flags, d_hists);
}
int ghf_planes_split_delta(ghf_ctx* c, const uint8_t* d_in, const uint8_t* d_base, size_t n_elems, uint32_t elem_bytes, uint8_t* d_planes,
                           size_t plane_stride) {
  return planes_split(c, "ghf_planes_split_delta", d_in, base_of(d_base), n_elems, elem_bytes, d_planes, plane_stride);
}
int ghf_planes_merge_delta(ghf_ctx* c, const uint8_t* d_planes, size_t plane_stride, const uint8_t* d_base, size_t n_elems,
                           uint32_t elem_bytes, uint8_t* d_out) {
  return planes_merge(c, "ghf_planes_merge_delta", d_planes, plane_stride, base_of(d_base), n_elems, elem_bytes, d_out);
}
int ghf_planes_merge_range_delta(ghf_ctx* c, const uint8_t* d_planes, size_t plane_stride, const uint8_t* d_base, size_t first, size_t count,
                                 uint32_t elem_bytes, uint8_t* d_out) {
  return planes_merge_range(c, "ghf_planes_merge_range_delta", d_planes, plane_stride, base_of(d_base), first, count, elem_bytes, d_out);
}
int ghf_compress_planes_delta(ghf_ctx* c, const uint8_t* d_in, const uint8_t* d_base, size_t n_elems, uint32_t elem_bytes, ghf_code* d_codes,
                              unsigned flags, uint8_t* d_out, size_t slot_bytes, uint64_t* d_out_bytes, const ghf_index* indexes) {
  return compress_planes_coded(c, "ghf_compress_planes_delta", d_in, base_of(d_base), n_elems, elem_bytes, d_codes, flags, d_out, slot_bytes,
                               d_out_bytes, indexes);
}
int ghf_decode_planes_delta(ghf_ctx* c, const uint8_t* const* h_stream_ptrs, const size_t* h_stream_bytes, const ghf_code* d_codes,
                            const ghf_index* indexes, const uint8_t* d_base, size_t n_elems, uint32_t elem_bytes, uint8_t* d_out, size_t cap,
                            uint64_t* d_out_bytes) {
  return decode_planes(c, "ghf_decode_planes_delta", h_stream_ptrs, h_stream_bytes, d_codes, indexes, base_of(d_base), n_elems, elem_bytes,
                       d_out, cap, d_out_bytes);
}
int ghf_decode_planes_range_delta(ghf_ctx* c, const uint8_t* const* h_stream_ptrs, const size_t* h_stream_bytes, const ghf_code* d_codes,
                                  const ghf_index* indexes, const ghf_seek_info* h_infos, const uint8_t* const* h_table_ptrs,
                                  const size_t* h_table_bytes, const uint8_t* d_base, uint32_t elem_bytes, uint64_t first, uint64_t count,
                                  uint8_t* d_out, size_t cap) {
  return decode_planes_range(c, "ghf_decode_planes_range_delta", h_stream_ptrs, h_stream_bytes, d_codes, indexes, h_infos, h_table_ptrs,
                             h_table_bytes, base_of(d_base), elem_bytes, first, count, d_out, cap);
}

// ---------------------------------------------------------------------------------------------- zero-suppressed byte planes
// (no reference counterpart)
size_t ghf_sparse_mask_bytes(size_t n) { return n / 8 + (n % 8 != 0); }

int ghf_sparse_split(ghf_ctx* c, const uint8_t* d_in, size_t n, uint8_t* d_mask, uint8_t* d_vals, size_t vals_cap, uint64_t* d_n_vals) {
  if (!c || !d_in || !d_mask || !d_n_vals || (vals_cap && !d_vals)) return GHF_E_INVAL;
  if (!aligned16(d_in) || !aligned16(d_mask) || !aligned16(d_vals) || (reinterpret_cast<uintptr_t>(d_n_vals) & 7u))
    return fail(c, GHF_E_INVAL, "ghf_sparse_split: d_in, d_mask and d_vals must be 16-byte aligned, d_n_vals 8-byte aligned");
  if (n > (size_t)-1 - kSparseTile) return fail(c, GHF_E_INVAL, "ghf_sparse_split: n overflows");
  if (n == 0) return fail(c, GHF_E_EMPTY, "ghf_sparse_split: no bytes");
  return queued(c, [&] {
    launch_sparse_split(d_in, n, d_mask, d_vals, vals_cap, d_n_vals, c->d_sparse_counts, c->d_sparse_offs, c->d_status, c->stream);
  });
}

int ghf_sparse_merge(ghf_ctx* c, const uint8_t* d_mask, const uint8_t* d_vals, size_t n_vals, size_t n, uint8_t* d_out) {
  if (!c || !d_mask || !d_out || (n_vals && !d_vals)) return GHF_E_INVAL;
  if (!aligned16(d_mask) || !aligned16(d_vals) || !aligned16(d_out))
    return fail(c, GHF_E_INVAL, "ghf_sparse_merge: d_mask, d_vals and d_out must be 16-byte aligned");
  if (n > (size_t)-1 - kSparseTile) return fail(c, GHF_E_INVAL, "ghf_sparse_merge: n overflows");
  if (n == 0) return fail(c, GHF_E_EMPTY, "ghf_sparse_merge: no bytes");
  return queued(c, [&] {
    launch_sparse_merge(d_mask, d_vals, n_vals, n, d_out, c->d_sparse_counts, c->d_sparse_offs, c->d_status, c->stream);
  });
}

static int compress_planes_sparse(ghf_ctx* c, const char* who, const uint8_t* d_in, Base base, size_t n_elems, uint32_t elem_bytes,
                                  unsigned sparse_planes, uint8_t* d_out, size_t slot_bytes, uint64_t* d_out_bytes, ghf_code* d_codes,
                                  ghf_index* h_indexes, unsigned* h_sparse_planes, size_t* h_n_vals, RankOut ranks) {
  if (!c || !d_in || !d_out || !d_out_bytes || !h_sparse_planes || !h_n_vals || base.null() || ranks.null()) return GHF_E_INVAL;
  const std::string f = std::string(who) + ": ";
  const uint32_t E = elem_bytes;
  const PlaneForms asked = {E, 0, sparse_planes, n_elems, h_n_vals};
  int rc = compress_args(c, f, kAlignedPlanes, d_in, base, d_out, slot_bytes, d_codes, ranks, n_elems, E, nullptr, [&] {
    return asked.sparse_planes_ok(true) ? nullptr : "sparse_planes is GHF_SPARSE_AUTO alone or has bits below elem_bytes only";
  });
  if (rc) return rc;
  GHF_HIP(c, hipSetDevice(c->device));
  size_t stride = 0, mask_stride = 0;
  rc = planes_workspace(c, n_elems, E, &stride);
  if (!rc) rc = sparse_workspace(c, n_elems, &mask_stride);
  if (!rc && !d_codes) rc = grow(c, c->batch_codes, 2 * GHF_PLANES_MAX);
  if (rc) return rc;
  ghf_code* codes = d_codes ? d_codes : c->batch_codes.p;
  // compressor.h:63 for all planes in one pass, and THE ONE WAIT of the call: count_p[0] says how many values plane p has
  if ((rc = histogram_planes_into(c, (f + "histogram launch").c_str(), d_in, base.p, n_elems, E, 0, c->d_planes_hists))) return rc;
  uint64_t counts[GHF_PLANES_MAX * GHF_NSYM];
  GHF_HIP(c, hipMemcpyAsync(counts, c->d_planes_hists, (size_t)E * GHF_NSYM * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  GHF_HIP(c, hipStreamSynchronize(c->stream));
  PlaneForms forms = {E, 0, 0, n_elems, h_n_vals};  // as chosen
  for (uint32_t p = 0; p < E; ++p) {
    const uint64_t zeros = counts[(size_t)p * GHF_NSYM];
    if (zeros > n_elems) return fail(c, GHF_E_HIP, (f + "the plane counts did not arrive").c_str());
    h_n_vals[p] = n_elems - (size_t)zeros;
    if (sparse_planes == GHF_SPARSE_AUTO ? zeros >= n_elems - n_elems / 4 : asked.is_sparse(p)) forms.store_sparse(p);
  }
  *h_sparse_planes = forms.sparse_planes;
  if ((rc = alloc_sidecars(c, forms, h_indexes))) return rc;
  GHF_HIP(c, hipMemsetAsync(d_out_bytes, 0, 2 * E * sizeof(uint64_t), c->stream));  // the empty slots
  launch_planes_split(d_in, base.p, n_elems, E, c->planes.p, stride, c->stream);
  GHF_HIP(c, hipGetLastError());
  const SlotsOut out = {d_out, slot_bytes, d_out_bytes, codes, h_indexes};
  for (uint32_t p = 0; p < E && !rc; ++p) {
    const uint8_t* plane = c->planes.p + p * stride;
    // K1 has not seen what stands at these addresses now: the workspaces are refilled for every plane
    c->hist.forget();
    c->plan.forget();
    if (forms.is_sparse(p)) {
      rc = pack_sparse_plane(c, plane, n_elems, h_n_vals[p], mask_stride, ranks.table(p), out, p, E);
    } else {  // what ghf_compress_planes_coded(GHF_PLANES_BUILD_CODES) queues for the plane
      if ((rc = ghf_build_codes(c, c->d_planes_hists + (size_t)p * GHF_NSYM, 1, codes + p, 0))) break;
      rc = pack_dense_plane(c, plane, n_elems, codes + p, out, p);
    }
  }
  c->hist.forget();
  c->plan.forget();
  return rc;
}

int ghf_compress_planes_sparse(ghf_ctx* c, const uint8_t* d_in, size_t n_elems, uint32_t elem_bytes, unsigned sparse_planes, uint8_t* d_out,
                               size_t slot_bytes, uint64_t* d_out_bytes, ghf_code* d_codes, ghf_index* h_indexes, unsigned* h_sparse_planes,
                               size_t* h_n_vals) {
  return compress_planes_sparse(c, "ghf_compress_planes_sparse", d_in, no_base(), n_elems, elem_bytes, sparse_planes, d_out, slot_bytes,
                                d_out_bytes, d_codes, h_indexes, h_sparse_planes, h_n_vals, no_ranks());
}
int ghf_compress_planes_sparse_delta(ghf_ctx* c, const uint8_t* d_in, const uint8_t* d_base, size_t n_elems, uint32_t elem_bytes,
                                     unsigned sparse_planes, uint8_t* d_out, size_t slot_bytes, uint64_t* d_out_bytes, ghf_code* d_codes,
                                     ghf_index* h_indexes, unsigned* h_sparse_planes, size_t* h_n_vals) {
  return compress_planes_sparse(c, "ghf_compress_planes_sparse_delta", d_in, base_of(d_base), n_elems, elem_bytes, sparse_planes, d_out,
                                slot_bytes, d_out_bytes, d_codes, h_indexes, h_sparse_planes, h_n_vals, no_ranks());
}

static int decode_planes_sparse(ghf_ctx* c, const char* who, const uint8_t* const* h_stream_ptrs, const size_t* h_stream_bytes,
                                const ghf_code* d_codes, const ghf_index* indexes, Base base, unsigned raw_planes, unsigned sparse_planes,
                                const size_t* h_n_vals, size_t n_elems, uint32_t elem_bytes, uint8_t* d_out, size_t cap,
                                uint64_t* d_out_bytes) {
  const uint32_t E = elem_bytes;
  const PlaneForms forms = {E, raw_planes, sparse_planes, n_elems, h_n_vals};
  // the codes of raw planes are not looked at: a tensor of nothing but raw planes needs none
  const bool all_raw = elem_bytes_ok(E) && forms.all_raw();
  if (!c || !h_stream_ptrs || !h_stream_bytes || (!d_codes && !all_raw) || !d_out || !h_n_vals || base.null()) return GHF_E_INVAL;
  const std::string f = std::string(who) + ": ";
  if (!elem_bytes_ok(E)) return fail(c, GHF_E_INVAL, (f + "elem_bytes must be 2, 4 or 8").c_str());
  if (!forms.sparse_planes_ok(false))
    return fail(c, GHF_E_INVAL, (f + "sparse_planes has bits below elem_bytes only (the mask the compress call reported)").c_str());
  if (!forms.forms_ok(false))
    return fail(c, GHF_E_INVAL, (f + "raw_planes has bits below elem_bytes only, none of them a sparse plane's").c_str());
  for (uint32_t p = 0; p < E; ++p)
    if (forms.is_sparse(p) && h_n_vals[p] > n_elems) return fail(c, GHF_E_INVAL, (f + "a plane has more values than elements").c_str());
  for (uint32_t j = 0; j < 2 * E; ++j)
    if (forms.stored(j) && (!h_stream_ptrs[j] || !aligned16(h_stream_ptrs[j])))
      return fail(c, GHF_E_INVAL, (f + "a stream pointer is null or not 16-byte aligned").c_str());
  if (!aligned16(d_out) || base.misaligned()) return fail(c, GHF_E_INVAL, (f + "d_out and d_base must be 16-byte aligned").c_str());
  if (workspace_overflow(n_elems, E)) return fail(c, GHF_E_INVAL, (f + "n_elems * elem_bytes overflows").c_str());
  for (uint32_t j = 0; indexes && j < 2 * E; ++j)
    if (forms.coded(j) && (indexes[j].n_symbols != forms.symbols(j) || !index_is_whole(&indexes[j])))
      return fail(c, GHF_E_INVAL, (f + "an index does not cover exactly the symbols of its stream").c_str());
  for (uint32_t p = 0; p < E; ++p)  // a raw plane is its n_elems bytes and nothing else
    if (forms.is_raw(p) && h_stream_bytes[p] != forms.symbols(p)) return fail(c, GHF_E_INVAL, (f + "a raw plane does not have n_elems bytes").c_str());
  if (n_elems == 0) return fail(c, GHF_E_EMPTY, (f + "no elements").c_str());
  if (cap < n_elems * E) return fail(c, GHF_E_CAP, (f + "output capacity below n_elems * elem_bytes").c_str());
  GHF_HIP(c, hipSetDevice(c->device));
  size_t stride = 0, mask_stride = 0;
  int rc = all_raw ? GHF_OK : planes_workspace(c, n_elems, E, &stride);
  if (!rc && sparse_planes) rc = sparse_workspace(c, n_elems, &mask_stride);
  if (rc) return rc;
  const std::string corrupt = f + "a stream does not decode to the size its plane gives it";
  // slot j of the caller's arrays into the workspace at d_to[0 .. room)
  const auto decode_slot = [&](uint32_t j, uint8_t* d_to, size_t room) {
    return decode_stored(c, corrupt, h_stream_ptrs[j], h_stream_bytes[j], d_codes + j, indexes ? indexes + j : nullptr, forms.symbols(j), d_to,
                         room);
  };
  for (uint32_t p = 0; p < E; ++p) {
    if (forms.is_raw(p)) continue;  // never copied: the merge reads it where it lies
    uint8_t* plane = c->planes.p + p * stride;
    if (!forms.is_sparse(p)) {
      if ((rc = decode_slot(p, plane, stride))) return rc;
      continue;
    }
    uint8_t *d_mask = c->sparse.p, *d_vals = c->sparse.p + mask_stride;
    if ((rc = decode_slot(p, d_mask, mask_stride))) return rc;
    if (forms.stored(E + p) && (rc = decode_slot(E + p, d_vals, c->sparse.cap - mask_stride))) return rc;
    launch_sparse_merge(d_mask, d_vals, h_n_vals[p], n_elems, plane, c->d_sparse_counts, c->d_sparse_offs, c->d_status, c->stream);
    GHF_HIP(c, hipGetLastError());
  }
  // nothing is stored behind a latched status
  if (!raw_planes) {
    launch_planes_merge(c->planes.p, stride, base.p, n_elems, E, d_out, c->d_status, c->stream);
  } else {
    const uint8_t* from[GHF_PLANES_MAX];
    for (uint32_t p = 0; p < E; ++p) from[p] = forms.is_raw(p) ? h_stream_ptrs[p] : c->planes.p + p * stride;
    launch_planes_merge_from(from, base.p, n_elems, E, d_out, c->d_status, c->stream);
  }
  if (d_out_bytes) launch_store_u64(d_out_bytes, nullptr, (uint64_t)n_elems * E, c->stream);
  GHF_HIP(c, hipGetLastError());
  return GHF_OK;
}

int ghf_decode_planes_sparse(ghf_ctx* c, const uint8_t* const* h_stream_ptrs, const size_t* h_stream_bytes, const ghf_code* d_codes,
                             const ghf_index* indexes, unsigned sparse_planes, const size_t* h_n_vals, size_t n_elems, uint32_t elem_bytes,
                             uint8_t* d_out, size_t cap, uint64_t* d_out_bytes) {
  return decode_planes_sparse(c, "ghf_decode_planes_sparse", h_stream_ptrs, h_stream_bytes, d_codes, indexes, no_base(), 0, sparse_planes,
                              h_n_vals, n_elems, elem_bytes, d_out, cap, d_out_bytes);
}
int ghf_decode_planes_sparse_delta(ghf_ctx* c, const uint8_t* const* h_stream_ptrs, const size_t* h_stream_bytes, const ghf_code* d_codes,
                                   const ghf_index* indexes, const uint8_t* d_base, unsigned sparse_planes, const size_t* h_n_vals,
                                   size_t n_elems, uint32_t elem_bytes, uint8_t* d_out, size_t cap, uint64_t* d_out_bytes) {
  return decode_planes_sparse(c, "ghf_decode_planes_sparse_delta", h_stream_ptrs, h_stream_bytes, d_codes, indexes, base_of(d_base), 0,
                              sparse_planes, h_n_vals, n_elems, elem_bytes, d_out, cap, d_out_bytes);
}

// ---------------------------------------------------------------------------------------------- element range of sparse planes
// (no reference counterpart)
size_t ghf_sparse_rank_bytes(size_t n) { return kSparseRankHeaderBytes + 8 * ((size_t)rank_blocks_for(n) + 1); }

int ghf_sparse_rank_pack(ghf_ctx* c, const uint8_t* d_mask, size_t n, uint8_t* d_table, size_t cap) {
  if (!c || !d_mask || !d_table) return GHF_E_INVAL;
  if (!aligned16(d_mask) || !aligned16(d_table)) return fail(c, GHF_E_INVAL, "ghf_sparse_rank_pack: d_mask and d_table must be 16-byte aligned");
  if (n > (size_t)-1 - kSparseRankElems) return fail(c, GHF_E_INVAL, "ghf_sparse_rank_pack: n overflows");
  if (n == 0) return fail(c, GHF_E_EMPTY, "ghf_sparse_rank_pack: no bytes");
  if (cap < ghf_sparse_rank_bytes(n)) return fail(c, GHF_E_CAP, "ghf_sparse_rank_pack: table capacity below ghf_sparse_rank_bytes(n)");
  return queued(c, [&] { launch_sparse_rank_pack(d_mask, n, d_table, c->d_sparse_counts, c->d_sparse_offs, c->d_status, c->stream); });
}

// The table is not trusted: everything one entry can be held against without the mask is checked here.  Whether the entries
// are the mask's own ranks is not: a range call holds the DIFFERENCE of the two entries it reads against the mask's set bits
// (the sparse merge's count) and nothing more, so two entries wrong by the same amount pass.
int ghf_sparse_rank_parse(const uint8_t* h, size_t bytes, ghf_sparse_rank_info* info) {
  if (!h || !info) return GHF_E_INVAL;
  std::memset(info, 0, sizeof *info);
  if (bytes < kSparseRankHeaderBytes + 8) return GHF_E_FORMAT;
  if (le64(h) != kSparseRankMagic || le32(h + 8) != kSparseRankVersion || le32(h + 12) != kSparseRankElems) return GHF_E_FORMAT;
  const uint64_t n = le64(h + 16), n_vals = le64(h + 24), nb = le64(h + 32);
  if (nb != rank_blocks_for(n) || n_vals > n) return GHF_E_FORMAT;
  for (size_t i = 40; i < kSparseRankHeaderBytes; ++i)
    if (h[i]) return GHF_E_FORMAT;
  if ((bytes - kSparseRankHeaderBytes) / 8 != nb + 1 || (bytes & 7u)) return GHF_E_FORMAT;  // truncated, or something behind it
  const uint8_t* cum = h + kSparseRankHeaderBytes;
  uint64_t prev = le64(cum);
  if (prev != 0) return GHF_E_FORMAT;
  for (uint64_t j = 1; j <= nb; ++j) {
    const uint64_t v = le64(cum + 8 * j), elems = j < nb ? kSparseRankElems : n - (nb - 1) * kSparseRankElems;
    if (v < prev || v - prev > elems) return GHF_E_FORMAT;  // a rank block has no more non-zero bytes than bytes
    prev = v;
  }
  if (prev != n_vals) return GHF_E_FORMAT;
  info->n = n;
  info->n_vals = n_vals;
  info->n_blocks = nb;
  info->version = kSparseRankVersion;
  return GHF_OK;
}

int ghf_sparse_merge_at(ghf_ctx* c, const uint8_t* d_mask, const uint8_t* d_vals, size_t vals_skip, size_t n_vals, size_t n, uint8_t* d_out) {
  if (!c || !d_mask || !d_out || (n_vals && !d_vals)) return GHF_E_INVAL;
  if (!aligned16(d_mask) || !aligned16(d_vals) || !aligned16(d_out))
    return fail(c, GHF_E_INVAL, "ghf_sparse_merge_at: d_mask, d_vals and d_out must be 16-byte aligned");
  if (n > (size_t)-1 - kSparseTile || vals_skip + n_vals < vals_skip) return fail(c, GHF_E_INVAL, "ghf_sparse_merge_at: n or vals_skip + n_vals overflows");
  if (n == 0) return fail(c, GHF_E_EMPTY, "ghf_sparse_merge_at: no bytes");
  return queued(c, [&] {
    launch_sparse_merge_at(d_mask, d_vals, vals_skip, n_vals, n, d_out, c->d_sparse_counts, c->d_sparse_offs, c->d_status, c->stream);
  });
}

int ghf_compress_planes_sparse_ranked(ghf_ctx* c, const uint8_t* d_in, size_t n_elems, uint32_t elem_bytes, unsigned sparse_planes,
                                      uint8_t* d_out, size_t slot_bytes, uint64_t* d_out_bytes, ghf_code* d_codes, ghf_index* h_indexes,
                                      unsigned* h_sparse_planes, size_t* h_n_vals, uint8_t* d_ranks, size_t rank_slot_bytes) {
  return compress_planes_sparse(c, "ghf_compress_planes_sparse_ranked", d_in, no_base(), n_elems, elem_bytes, sparse_planes, d_out, slot_bytes,
                                d_out_bytes, d_codes, h_indexes, h_sparse_planes, h_n_vals, {true, d_ranks, rank_slot_bytes});
}
int ghf_compress_planes_sparse_ranked_delta(ghf_ctx* c, const uint8_t* d_in, const uint8_t* d_base, size_t n_elems, uint32_t elem_bytes,
                                            unsigned sparse_planes, uint8_t* d_out, size_t slot_bytes, uint64_t* d_out_bytes,
                                            ghf_code* d_codes, ghf_index* h_indexes, unsigned* h_sparse_planes, size_t* h_n_vals,
                                            uint8_t* d_ranks, size_t rank_slot_bytes) {
  return compress_planes_sparse(c, "ghf_compress_planes_sparse_ranked_delta", d_in, base_of(d_base), n_elems, elem_bytes, sparse_planes, d_out,
                                slot_bytes, d_out_bytes, d_codes, h_indexes, h_sparse_planes, h_n_vals, {true, d_ranks, rank_slot_bytes});
}

static int decode_planes_sparse_range(ghf_ctx* c, const char* who, const uint8_t* const* h_stream_ptrs, const size_t* h_stream_bytes,
                                      const ghf_code* d_codes, const ghf_index* indexes, const ghf_seek_info* h_infos,
                                      const uint8_t* const* h_table_ptrs, const size_t* h_table_bytes,
                                      const ghf_sparse_rank_info* h_rank_infos, const uint8_t* const* h_rank_ptrs, Base base,
                                      unsigned raw_planes, unsigned sparse_planes, size_t n_elems, uint32_t elem_bytes, uint64_t first,
                                      uint64_t count, uint8_t* d_out, size_t cap) {
  const uint32_t E = elem_bytes;
  const StoredStreams s = {h_stream_ptrs, h_stream_bytes, d_codes, indexes, h_infos, h_table_ptrs, h_table_bytes};
  size_t n_vals[GHF_PLANES_MAX] = {};  // of the sparse planes: what their rank infos count, once those are checked
  const PlaneForms forms = {E, raw_planes, sparse_planes, n_elems, n_vals};
  // the codes of raw planes are not looked at: a tensor of nothing but raw planes needs none
  const bool all_raw = elem_bytes_ok(E) && forms.all_raw();
  if (!c || !h_stream_ptrs || !h_stream_bytes || (!d_codes && !all_raw) || !d_out || base.null()) return GHF_E_INVAL;
  const std::string f = std::string(who) + ": ";
  if (!elem_bytes_ok(E)) return fail(c, GHF_E_INVAL, (f + "elem_bytes must be 2, 4 or 8").c_str());
  if (!s.one_source())
    return fail(c, GHF_E_INVAL, (f + "exactly one of indexes / (h_infos, h_table_ptrs, h_table_bytes) must be given").c_str());
  const bool by_table = s.by_table();
  // What the dense range asks of a plane (decode_planes_range_checks), of one stored stream.  A raw plane
  // has a stream pointer and a size and nothing else: its index, info and table are not read
  auto pointers_ok = [&](uint32_t j) {
    return h_stream_ptrs[j] && aligned16(h_stream_ptrs[j]) &&
           (!by_table || forms.is_raw(j) || (h_table_ptrs[j] && aligned16(h_table_ptrs[j])));
  };
  for (uint32_t p = 0; p < E; ++p)
    if (!pointers_ok(p)) return fail(c, GHF_E_INVAL, (f + "a stream or table pointer is null or not 16-byte aligned").c_str());
  if (!aligned16(d_out) || base.misaligned()) return fail(c, GHF_E_INVAL, (f + "d_out and d_base must be 16-byte aligned").c_str());
  for (uint32_t p = 0; p < E; ++p)
    if (!forms.is_raw(p) && !s.index_ok(p)) return fail(c, GHF_E_INVAL, (f + "malformed index").c_str());
  if (first > n_elems || count > n_elems - first) return fail(c, GHF_E_INVAL, (f + "first + count exceeds n_elems").c_str());
  // the workspace holds the range from the start of its first rank block to the end of its last, and a vector more
  const size_t slack = 2 * (size_t)kSparseRankElems + 16;
  if (count > (size_t)-1 - slack || workspace_overflow((size_t)count + slack, E))
    return fail(c, GHF_E_INVAL, (f + "count * elem_bytes overflows").c_str());
  for (uint32_t p = 0; by_table && p < E; ++p) {
    if (forms.is_raw(p)) continue;
    const int rc = seek_table_ok(c, who, h_infos + p, h_table_ptrs[p], h_table_bytes[p]);
    if (rc) return rc;
  }
  if (cap < count * E) return fail(c, GHF_E_CAP, (f + "output capacity below count * elem_bytes").c_str());
  // ... and what the sparse form adds
  if (!forms.sparse_planes_ok(false))
    return fail(c, GHF_E_INVAL, (f + "sparse_planes has bits below elem_bytes only (the mask the compress call reported)").c_str());
  // ... and the raw form
  if (!forms.forms_ok(false))
    return fail(c, GHF_E_INVAL, (f + "raw_planes has bits below elem_bytes only, none of them a sparse plane's").c_str());
  for (uint32_t p = 0; p < E; ++p)
    if (forms.is_raw(p) && h_stream_bytes[p] != n_elems) return fail(c, GHF_E_INVAL, (f + "a raw plane does not have n_elems bytes").c_str());
  if (sparse_planes && (!h_rank_infos || !h_rank_ptrs)) return fail(c, GHF_E_INVAL, (f + "sparse planes need their rank tables").c_str());
  for (uint32_t p = 0; p < E; ++p) {
    if (!forms.is_sparse(p)) continue;
    if (!h_rank_ptrs[p]) return fail(c, GHF_E_INVAL, (f + "a sparse plane has no rank table").c_str());
    if (h_rank_infos[p].n != n_elems) return fail(c, GHF_E_INVAL, (f + "a rank table is not one of n_elems elements").c_str());
    if (h_rank_infos[p].version != kSparseRankVersion || h_rank_infos[p].n_blocks != rank_blocks_for(n_elems) || h_rank_infos[p].n_vals > n_elems)
      return fail(c, GHF_E_FORMAT, (f + "a rank info is not what ghf_sparse_rank_parse fills in").c_str());
    n_vals[p] = (size_t)h_rank_infos[p].n_vals;
  }
  for (uint32_t p = 0; p < E; ++p) {
    if (forms.is_raw(p)) continue;
    if (s.symbols(p) != forms.symbols(p))
      return fail(c, GHF_E_INVAL, forms.is_sparse(p) ? (f + "a mask stream does not have ghf_sparse_mask_bytes(n_elems) symbols").c_str()
                                                     : (f + "a dense stream does not have n_elems symbols").c_str());
    if (!forms.stored(E + p)) continue;  // the values slot of any other plane is ignored
    if (!pointers_ok(E + p)) return fail(c, GHF_E_INVAL, (f + "a stream or table pointer is null or not 16-byte aligned").c_str());
    if (!s.index_ok(E + p)) return fail(c, GHF_E_INVAL, (f + "malformed index").c_str());
    if (s.symbols(E + p) != forms.symbols(E + p))
      return fail(c, GHF_E_INVAL, (f + "a values stream does not have the symbols its rank table counts").c_str());
    if (by_table) {
      const int rc = seek_table_ok(c, who, h_infos + E + p, h_table_ptrs[E + p], h_table_bytes[E + p]);
      if (rc) return rc;
    }
  }
  if (count == 0) return GHF_OK;
  if (!sparse_planes && !raw_planes)  // nothing sparse or raw: the origin of section 17, and its work -- every check of it is made
    return decode_planes_range_work(c, s, base, E, first, count, d_out);
  // THE PLAN.  The common origin of all planes is the start of the rank block that holds `first`: a multiple of 4096 for a
  // dense plane, of 4096 mask bytes for a mask, and the values in front of it number cum[b0].  A sparse plane is rebuilt for the
  // whole rank blocks [b0, b1) (cut at n_elems): the sub-string's mask bytes are whole, so its last mask byte obeys the pad rule.
  // With raw planes and no sparse one the origin is section 17's, the start of the seek block that holds `first`.  A raw plane has
  // no part in the plan: nothing of it is decoded or copied, the merge reads it at stream + first.
  const uint64_t origin = sparse_planes ? kSparseRankElems : kBlockSymbols;
  const uint64_t from = first - first % origin, end = first + count;
  const uint64_t b0 = from / kSparseRankElems, b1 = rank_blocks_for(end);
  const uint64_t sub_n = (sparse_planes ? std::min<uint64_t>(b1 * kSparseRankElems, n_elems) : end) - from;
  const uint64_t m_lo = b0 * (kSparseRankElems / 8), m_hi = std::min<uint64_t>(b1 * (kSparseRankElems / 8), forms.mask_bytes());
  uint64_t v_lo[GHF_PLANES_MAX] = {}, v_hi[GHF_PLANES_MAX] = {};
  for (uint32_t p = 0; p < E; ++p) {
    if (!forms.is_sparse(p)) continue;
    const uint8_t* cum = h_rank_ptrs[p] + kSparseRankHeaderBytes;
    v_lo[p] = le64(cum + 8 * b0);
    v_hi[p] = le64(cum + 8 * b1);
    if (v_lo[p] > v_hi[p] || v_hi[p] > n_vals[p] || v_hi[p] - v_lo[p] > sub_n)
      return fail(c, GHF_E_FORMAT, (f + "the rank table's entries for the range are not ordered ranks").c_str());
  }
  GHF_HIP(c, hipSetDevice(c->device));
  size_t stride = 0;
  int rc = all_raw ? GHF_OK : planes_workspace(c, (size_t)sub_n + 16, E, &stride);
  // the second workspace: the sub-string's mask, and behind it its values from the start of their first seek block
  const size_t mask_stride = ((size_t)(m_hi - m_lo) + 255) & ~(size_t)255;
  const size_t vals_room = ((size_t)sub_n + kBlockSymbols + 255) & ~(size_t)255;
  if (!rc && sparse_planes) rc = grow(c, c->sparse, mask_stride + vals_room);
  if (rc) return rc;
  uint8_t *d_mask = c->sparse.p, *d_vals = c->sparse.p + mask_stride;
  RangePart parts[2 * GHF_PLANES_MAX];
  uint32_t n_parts = 0;
  for (uint32_t p = 0; p < E; ++p) {
    if (forms.is_raw(p)) continue;
    if (!forms.is_sparse(p)) {
      parts[n_parts++] = {p, from, end, forms.symbols(p), c->planes.p + p * stride, stride};
      continue;
    }
    parts[n_parts++] = {p, m_lo, m_hi, forms.symbols(p), d_mask, mask_stride};
    if (v_hi[p] > v_lo[p]) parts[n_parts++] = {E + p, v_lo[p] - v_lo[p] % kBlockSymbols, v_hi[p], forms.symbols(E + p), d_vals, vals_room};
  }
  // behind the last stored stream of a sparse plane (its values, or its mask when the sub-string has none): the plane's merge
  auto merge_behind = [&](uint32_t j) {
    const uint32_t p = j % E;
    if (forms.is_sparse(p) && (j >= E || v_hi[p] == v_lo[p]))
      launch_sparse_merge_at(d_mask, d_vals, v_lo[p] % kBlockSymbols, v_hi[p] - v_lo[p], sub_n, c->planes.p + p * stride, c->d_sparse_counts,
                             c->d_sparse_offs, c->d_status, c->stream);
  };
  // from tables: every stored stream gets tables of its own, in one launch, and one launch expands the covered blocks of all
  // of them (k_seek_expand_streams)
  const auto expand = [&](const SeekExpandParams* x, uint32_t n) {
    SeekExpandStreamsParams a = {};
    std::copy(x, x + n, a.stream);
    uint32_t slots = 0;
    for (uint32_t i = 0; i < n; ++i) slots |= 1u << parts[i].slot;
    launch_build_decode_tables_slots(d_codes, c->range_dt.p, 2 * E, slots, c->d_status, c->stream);
    launch_seek_expand_streams(a, n, c->stream);
    GHF_HIP(c, hipGetLastError());
    return (int)GHF_OK;
  };
  // with every plane raw there is no part, and the merge below is the whole call
  if (n_parts && (rc = decode_parts(c, s, parts, n_parts, 2 * GHF_PLANES_MAX, expand, merge_behind))) return rc;
  // nothing reaches d_out behind a failed decode or a count that does not match the rank table
  if (!raw_planes) {
    launch_planes_merge_range(c->planes.p, stride, base.p, first - from, count, E, d_out, c->d_status, c->stream);
  } else {
    // the workspace planes start 256-byte aligned at element `from`, a multiple of 4096, and a raw plane 16-byte aligned at
    // element 0: the run's first byte stands first % 16 behind a vector in every one of them
    const uint8_t* src[GHF_PLANES_MAX];
    for (uint32_t p = 0; p < E; ++p) src[p] = forms.is_raw(p) ? h_stream_ptrs[p] + first : c->planes.p + p * stride + (first - from);
    launch_planes_merge_from(src, base.p, count, E, d_out, c->d_status, c->stream);
  }
  GHF_HIP(c, hipGetLastError());
  return GHF_OK;
}

int ghf_decode_planes_sparse_range(ghf_ctx* c, const uint8_t* const* h_stream_ptrs, const size_t* h_stream_bytes, const ghf_code* d_codes,
                                   const ghf_index* indexes, const ghf_seek_info* h_infos, const uint8_t* const* h_table_ptrs,
                                   const size_t* h_table_bytes, const ghf_sparse_rank_info* h_rank_infos, const uint8_t* const* h_rank_ptrs,
                                   unsigned sparse_planes, size_t n_elems, uint32_t elem_bytes, uint64_t first, uint64_t count, uint8_t* d_out,
                                   size_t cap) {
  return decode_planes_sparse_range(c, "ghf_decode_planes_sparse_range", h_stream_ptrs, h_stream_bytes, d_codes, indexes, h_infos, h_table_ptrs,
                                    h_table_bytes, h_rank_infos, h_rank_ptrs, no_base(), 0, sparse_planes, n_elems, elem_bytes, first, count,
                                    d_out, cap);
}
int ghf_decode_planes_sparse_range_delta(ghf_ctx* c, const uint8_t* const* h_stream_ptrs, const size_t* h_stream_bytes, const ghf_code* d_codes,
                                         const ghf_index* indexes, const ghf_seek_info* h_infos, const uint8_t* const* h_table_ptrs,
                                         const size_t* h_table_bytes, const ghf_sparse_rank_info* h_rank_infos,
                                         const uint8_t* const* h_rank_ptrs, const uint8_t* d_base, unsigned sparse_planes, size_t n_elems,
                                         uint32_t elem_bytes, uint64_t first, uint64_t count, uint8_t* d_out, size_t cap) {
  return decode_planes_sparse_range(c, "ghf_decode_planes_sparse_range_delta", h_stream_ptrs, h_stream_bytes, d_codes, indexes, h_infos,
                                    h_table_ptrs, h_table_bytes, h_rank_infos, h_rank_ptrs, base_of(d_base), 0, sparse_planes, n_elems,
                                    elem_bytes, first, count, d_out, cap);
}

// ---------------------------------------------------------------------------------------------- byte planes in three forms
// (no reference counterpart).  In this family d_base is optional: null is the plain call (base_opt)
// what the three pointer calls check alike: `d_inter` is the interleaved side, `h_ptrs` the host array of plane addresses;
// *skew <- their common address mod 16 (the split wants 0)
static int plane_ptrs_args(ghf_ctx* c, const char* who, const uint8_t* d_inter, const uint8_t* const* h_ptrs, const uint8_t* d_base,
                           size_t n_elems, uint32_t elem_bytes, uint32_t* skew) {
  if (!c || !d_inter || !h_ptrs) return GHF_E_INVAL;
  const std::string f = std::string(who) + ": ";
  if (!elem_bytes_ok(elem_bytes)) return fail(c, GHF_E_INVAL, (f + "elem_bytes must be 2, 4 or 8").c_str());
  for (uint32_t p = 0; p < elem_bytes; ++p)
    if (!h_ptrs[p]) return fail(c, GHF_E_INVAL, (f + "a plane pointer is null").c_str());
  *skew = (uint32_t)(reinterpret_cast<uintptr_t>(h_ptrs[0]) & 15u);
  for (uint32_t p = 1; p < elem_bytes; ++p)
    if ((reinterpret_cast<uintptr_t>(h_ptrs[p]) & 15u) != *skew)
      return fail(c, GHF_E_INVAL, (f + "the plane pointers do not have the same address modulo 16").c_str());
  if (!aligned16(d_inter) || !aligned16(d_base)) return fail(c, GHF_E_INVAL, (f + "d_in / d_out and d_base must be 16-byte aligned").c_str());
  if (elems_overflow(n_elems, elem_bytes)) return fail(c, GHF_E_INVAL, (f + "n_elems * elem_bytes overflows").c_str());
  if (n_elems == 0) return fail(c, GHF_E_EMPTY, (f + "no elements").c_str());
  return GHF_OK;
}

int ghf_planes_split_to(ghf_ctx* c, const uint8_t* d_in, const uint8_t* d_base, size_t n_elems, uint32_t elem_bytes,
                        uint8_t* const* h_plane_ptrs) {
  uint32_t skew = 0;
  const int rc = plane_ptrs_args(c, "ghf_planes_split_to", d_in, h_plane_ptrs, d_base, n_elems, elem_bytes, &skew);
  if (rc) return rc;
  if (skew) return fail(c, GHF_E_INVAL, "ghf_planes_split_to: the plane pointers must be 16-byte aligned");
  return queued(c, [&] { launch_planes_split_to(d_in, d_base, n_elems, elem_bytes, h_plane_ptrs, c->stream); });
}

int ghf_planes_merge_from(ghf_ctx* c, const uint8_t* const* h_plane_ptrs, const uint8_t* d_base, size_t n_elems, uint32_t elem_bytes,
                          uint8_t* d_out) {
  uint32_t skew = 0;
  const int rc = plane_ptrs_args(c, "ghf_planes_merge_from", d_out, h_plane_ptrs, d_base, n_elems, elem_bytes, &skew);
  if (rc) return rc;
  if (skew) return fail(c, GHF_E_INVAL, "ghf_planes_merge_from: the plane pointers must be 16-byte aligned");
  return queued(c, [&] { launch_planes_merge_from(h_plane_ptrs, d_base, n_elems, elem_bytes, d_out, nullptr, c->stream); });
}

int ghf_planes_merge_range_from(ghf_ctx* c, const uint8_t* const* h_plane_ptrs, const uint8_t* d_base, size_t count, uint32_t elem_bytes,
                                uint8_t* d_out) {
  uint32_t skew = 0;
  const int rc = plane_ptrs_args(c, "ghf_planes_merge_range_from", d_out, h_plane_ptrs, d_base, count, elem_bytes, &skew);
  if (rc) return rc;
  return queued(c, [&] {  // the common skew picks the kernel
    launch_planes_merge_from(h_plane_ptrs, d_base, count, elem_bytes, d_out, nullptr, c->stream);
  });
}

int ghf_compress_planes_forms(ghf_ctx* c, const uint8_t* d_in, const uint8_t* d_base, size_t n_elems, uint32_t elem_bytes,
                              unsigned raw_planes, unsigned sparse_planes, uint8_t* d_out, size_t slot_bytes, uint64_t* d_out_bytes,
                              ghf_code* d_codes, ghf_index* h_indexes, uint8_t* d_ranks, size_t rank_slot_bytes, unsigned* h_raw_planes,
                              unsigned* h_sparse_planes, size_t* h_n_vals) {
  return compress_planes_forms(c, "ghf_compress_planes_forms", d_in, d_base, n_elems, elem_bytes, raw_planes, sparse_planes, d_out,
                               slot_bytes, d_out_bytes, d_codes, h_indexes, false, d_ranks, rank_slot_bytes, h_raw_planes, h_sparse_planes,
                               h_n_vals);
}

}  // extern "C"

// the driver of the call above, under the caller's name: ghf_compress_tensor (ghf_api_tensor.hip) runs it with pooled side-cars
int ghf::compress_planes_forms(ghf_ctx* c, const char* who, const uint8_t* d_in, const uint8_t* d_base, size_t n_elems, uint32_t elem_bytes,
                               unsigned raw_planes, unsigned sparse_planes, uint8_t* d_out, size_t slot_bytes, uint64_t* d_out_bytes,
                               ghf_code* d_codes, ghf_index* h_indexes, bool pooled, uint8_t* d_ranks, size_t rank_slot_bytes,
                               unsigned* h_raw_planes, unsigned* h_sparse_planes, size_t* h_n_vals) {
  if (!c || !d_in || !d_out || !d_out_bytes || !h_raw_planes || !h_sparse_planes || !h_n_vals) return GHF_E_INVAL;
  const std::string f = std::string(who) + ": ";
  const uint32_t E = elem_bytes;
  const PlaneForms asked = {E, raw_planes, sparse_planes, n_elems, h_n_vals};
  const RankOut ranks = {d_ranks != nullptr, d_ranks, rank_slot_bytes};  // optional too
  int rc = compress_args(c, f, kAlignedPlanes, d_in, base_opt(d_base), d_out, slot_bytes, d_codes, ranks, n_elems, E, nullptr,
                         [&]() -> const char* {
                           if (!asked.sparse_planes_ok(true)) return "sparse_planes is GHF_SPARSE_AUTO alone or has bits below elem_bytes only";
                           if (!asked.forms_ok(true))
                             return "raw_planes is GHF_RAW_AUTO alone or has bits below elem_bytes only, none of them a sparse plane's";
                           return nullptr;
                         });
  if (rc) return rc;
  GHF_HIP(c, hipSetDevice(c->device));
  const bool raw_auto = raw_planes == GHF_RAW_AUTO, sparse_auto = sparse_planes == GHF_SPARSE_AUTO;
  // the counts are needed on the HOST for a choice and for the value counts of sparse planes, on the device for every code
  const bool wait = raw_auto || sparse_auto || sparse_planes != 0;
  // [0, 2 MAX): the codes of the stored streams when the caller wants none; [2 MAX, 3 MAX): the codes the choice is priced with
  if ((rc = grow(c, c->batch_codes, 3 * GHF_PLANES_MAX))) return rc;
  ghf_code* codes = d_codes ? d_codes : c->batch_codes.p;
  ghf_code* priced = c->batch_codes.p + 2 * GHF_PLANES_MAX;
  uint64_t* d_prices = c->d_planes_hists + (size_t)GHF_PLANES_MAX * GHF_NSYM;
  if (wait || !asked.all_raw())
    if ((rc = histogram_planes_into(c, (f + "histogram launch").c_str(), d_in, d_base, n_elems, E, 0, c->d_planes_hists))) return rc;
  PlaneForms forms = {E, raw_auto ? 0u : raw_planes, sparse_auto ? 0u : sparse_planes, n_elems, h_n_vals};  // as chosen
  std::memset(h_n_vals, 0, E * sizeof *h_n_vals);
  if (wait) {
    // THE ONE WAIT of the call.  With GHF_RAW_AUTO the codes of all planes and the sizes of their images are queued in front of
    // it, and one copy brings the counts and the sizes back; the dense planes are then packed with those codes
    if (raw_auto) {
      if ((rc = ghf_build_codes(c, c->d_planes_hists, E, priced, 0))) return rc;
      launch_planes_image_bytes(c->d_planes_hists, priced, E, d_prices, c->stream);
      GHF_HIP(c, hipGetLastError());
    }
    uint64_t got[GHF_PLANES_MAX * GHF_NSYM + GHF_PLANES_MAX];
    GHF_HIP(c, hipMemcpyAsync(got, c->d_planes_hists, sizeof got, hipMemcpyDeviceToHost, c->stream));
    GHF_HIP(c, hipStreamSynchronize(c->stream));
    const uint64_t* prices = got + (size_t)GHF_PLANES_MAX * GHF_NSYM;
    // a sparse plane stores two headers: at or below that size the raw form is the smaller one whatever the plane holds
    const bool sparse_pays = !raw_auto || n_elems > 2 * ghf_header_bytes(1);
    for (uint32_t p = 0; p < E; ++p) {
      const uint64_t zeros = got[(size_t)p * GHF_NSYM];
      if (zeros > n_elems) return fail(c, GHF_E_HIP, (f + "the plane counts did not arrive").c_str());
      h_n_vals[p] = n_elems - (size_t)zeros;
      if (sparse_auto && !forms.is_raw(p) && sparse_pays && zeros >= n_elems - n_elems / 4) forms.store_sparse(p);
      // prices[p] == 0: the plane has no code (a count at or above 2^55); it stays dense, and the dense path latches why
      if (raw_auto && !forms.is_sparse(p) && prices[p] >= n_elems) forms.store_raw(p);
    }
  }
  *h_raw_planes = forms.raw_planes;
  *h_sparse_planes = forms.sparse_planes;
  size_t stride = 0, mask_stride = 0;
  if (!forms.all_raw()) rc = planes_workspace(c, n_elems, E, &stride);
  if (!rc && forms.sparse_planes) rc = sparse_workspace(c, n_elems, &mask_stride);
  if (rc) return rc;
  if ((rc = alloc_sidecars(c, forms, h_indexes, pooled))) return rc;
  GHF_HIP(c, hipMemsetAsync(d_out_bytes, 0, 2 * E * sizeof(uint64_t), c->stream));  // the empty slots
  const SlotsOut out = {d_out, slot_bytes, d_out_bytes, codes, h_indexes};
  // the split writes a raw plane straight into its slot and every other plane into the workspace
  if (!forms.raw_planes) {
    launch_planes_split(d_in, d_base, n_elems, E, c->planes.p, stride, c->stream);
  } else {
    uint8_t* to[GHF_PLANES_MAX];
    for (uint32_t p = 0; p < E; ++p) to[p] = forms.is_raw(p) ? out.image(p) : c->planes.p + p * stride;
    launch_planes_split_to(d_in, d_base, n_elems, E, to, c->stream);
  }
  GHF_HIP(c, hipGetLastError());
  for (uint32_t p = 0; p < E && !rc; ++p) {
    if (forms.is_raw(p)) {
      launch_store_u64(d_out_bytes + p, nullptr, (uint64_t)forms.symbols(p), c->stream);
      GHF_HIP(c, hipGetLastError());
      continue;
    }
    const uint8_t* plane = c->planes.p + p * stride;
    // K1 has not seen what stands at these addresses now: the workspaces are refilled for every plane
    c->hist.forget();
    c->plan.forget();
    if (forms.is_sparse(p)) {
      rc = pack_sparse_plane(c, plane, n_elems, h_n_vals[p], mask_stride, ranks.table(p), out, p, E);
      continue;
    }
    // what ghf_compress_planes_coded(GHF_PLANES_BUILD_CODES) queues for the plane -- with GHF_RAW_AUTO under the code it was priced with
    const ghf_code* code = raw_auto ? priced + p : codes + p;
    if (!raw_auto && (rc = ghf_build_codes(c, c->d_planes_hists + (size_t)p * GHF_NSYM, 1, codes + p, 0))) break;
    if ((rc = pack_dense_plane(c, plane, n_elems, code, out, p))) break;
    if (raw_auto && d_codes) GHF_HIP(c, hipMemcpyAsync(d_codes + p, code, sizeof(ghf_code), hipMemcpyDeviceToDevice, c->stream));
  }
  c->hist.forget();
  c->plan.forget();
  return rc;
}

extern "C" {

int ghf_decode_planes_forms(ghf_ctx* c, const uint8_t* const* h_stream_ptrs, const size_t* h_stream_bytes, const ghf_code* d_codes,
                            const ghf_index* indexes, const uint8_t* d_base, unsigned raw_planes, unsigned sparse_planes,
                            const size_t* h_n_vals, size_t n_elems, uint32_t elem_bytes, uint8_t* d_out, size_t cap, uint64_t* d_out_bytes) {
  return decode_planes_sparse(c, "ghf_decode_planes_forms", h_stream_ptrs, h_stream_bytes, d_codes, indexes, base_opt(d_base), raw_planes,
                              sparse_planes, h_n_vals, n_elems, elem_bytes, d_out, cap, d_out_bytes);
}

int ghf_decode_planes_forms_range(ghf_ctx* c, const uint8_t* const* h_stream_ptrs, const size_t* h_stream_bytes, const ghf_code* d_codes,
                                  const ghf_index* indexes, const ghf_seek_info* h_infos, const uint8_t* const* h_table_ptrs,
                                  const size_t* h_table_bytes, const ghf_sparse_rank_info* h_rank_infos, const uint8_t* const* h_rank_ptrs,
                                  const uint8_t* d_base, unsigned raw_planes, unsigned sparse_planes, size_t n_elems, uint32_t elem_bytes,
                                  uint64_t first, uint64_t count, uint8_t* d_out, size_t cap) {
  return decode_planes_sparse_range(c, "ghf_decode_planes_forms_range", h_stream_ptrs, h_stream_bytes, d_codes, indexes, h_infos,
                                    h_table_ptrs, h_table_bytes, h_rank_infos, h_rank_ptrs, base_opt(d_base), raw_planes, sparse_planes,
                                    n_elems, elem_bytes, first, count, d_out, cap);
}

// ------------------------------------------------------------------------------------------ many rows in one call
// (no reference counterpart).  One launch whatever n_rows is; the rows' failures are their own
// (d_row_status) and nothing here or on the device touches the context's status word.
// what the two gather calls refuse alike, in this order (include/ghf.h), over the planes' own slots j < elem_bytes: `sparse` names
// the planes whose slot holds a mask -- a stream with a code and a table like a dense plane's, but of another symbol count,
// which the forms call holds against the mask's size behind its own masks -- and sets the row cap
static int gather_args(ghf_ctx* c, const char* who, const uint8_t* const* h_stream_ptrs, const size_t* h_stream_bytes, const ghf_code* d_codes,
                       const ghf_seek_info* h_infos, const uint8_t* const* h_table_ptrs, const size_t* h_table_bytes, unsigned raw_planes,
                       unsigned sparse, size_t n_elems, uint32_t elem_bytes, const uint64_t* d_index, uint32_t row_elems, const uint8_t* d_out,
                       size_t out_stride, const int32_t* d_row_status) {
  const std::string f = std::string(who) + ": ";
  const uint32_t E = elem_bytes;
  if (!elem_bytes_ok(E)) return fail(c, GHF_E_INVAL, (f + "elem_bytes must be 2, 4 or 8").c_str());
  const PlaneForms forms = {E, raw_planes, 0, n_elems, nullptr};
  if ((raw_planes >> E) != 0) return fail(c, GHF_E_INVAL, (f + "raw_planes has bits below elem_bytes only").c_str());
  if (row_elems == 0 || row_elems > (sparse ? GHF_GATHER_SPARSE_MAX_ROW_ELEMS : GHF_GATHER_MAX_ROW_ELEMS))
    return fail(c, GHF_E_INVAL, sparse ? (f + "row_elems must be 1 .. GHF_GATHER_SPARSE_MAX_ROW_ELEMS with a sparse plane").c_str()
                                       : (f + "row_elems must be 1 .. GHF_GATHER_MAX_ROW_ELEMS").c_str());
  if (out_stride < (size_t)row_elems * E) return fail(c, GHF_E_INVAL, (f + "out_stride below row_elems * elem_bytes").c_str());
  // the codes and tables of raw planes are not looked at: a tensor of nothing but raw planes needs none
  const bool all_raw = forms.all_raw();
  if (!h_stream_ptrs || !h_stream_bytes || !d_index || !d_out || !d_row_status ||
      (!all_raw && (!d_codes || !h_infos || !h_table_ptrs || !h_table_bytes)))
    return fail(c, GHF_E_INVAL, (f + "a required pointer is null").c_str());
  for (uint32_t p = 0; p < E; ++p)
    if (!h_stream_ptrs[p] || !aligned16(h_stream_ptrs[p]) || (!forms.is_raw(p) && (!h_table_ptrs[p] || !aligned16(h_table_ptrs[p]))))
      return fail(c, GHF_E_INVAL, (f + "a stream or table pointer is null or not 16-byte aligned").c_str());
  if (!aligned16(d_out) || !aligned16(d_codes) || (reinterpret_cast<uintptr_t>(d_index) & 7u) || (reinterpret_cast<uintptr_t>(d_row_status) & 3u))
    return fail(c, GHF_E_INVAL, (f + "d_out and d_codes must be 16-byte, d_index 8-byte and d_row_status 4-byte aligned").c_str());
  for (uint32_t p = 0; p < E; ++p)
    if (forms.is_raw(p) && h_stream_bytes[p] != n_elems) return fail(c, GHF_E_INVAL, (f + "a raw plane does not have n_elems bytes").c_str());
  for (uint32_t p = 0; p < E; ++p) {
    if (forms.is_raw(p)) continue;
    if (!(sparse >> p & 1u) && h_infos[p].n_symbols != n_elems)
      return fail(c, GHF_E_INVAL, (f + "a dense stream does not have n_elems symbols").c_str());
    const int rc = seek_table_ok(c, who, h_infos + p, h_table_ptrs[p], h_table_bytes[p]);
    if (rc) return rc;
  }
  return GHF_OK;
}

int ghf_decode_planes_gather(ghf_ctx* c, const uint8_t* const* h_stream_ptrs, const size_t* h_stream_bytes, const ghf_code* d_codes,
                             const ghf_seek_info* h_infos, const uint8_t* const* h_table_ptrs, const size_t* h_table_bytes,
                             unsigned raw_planes, size_t n_elems, uint32_t elem_bytes, const uint64_t* d_index, uint64_t index_stride,
                             uint32_t row_elems, uint32_t n_rows, uint8_t* d_out, size_t out_stride, int32_t* d_row_status) {
  if (!c) return GHF_E_INVAL;
  const uint32_t E = elem_bytes;
  const int rc = gather_args(c, "ghf_decode_planes_gather", h_stream_ptrs, h_stream_bytes, d_codes, h_infos, h_table_ptrs, h_table_bytes,
                             raw_planes, 0, n_elems, E, d_index, row_elems, d_out, out_stride, d_row_status);
  if (rc) return rc;
  if (n_rows == 0) return GHF_OK;
  const PlaneForms forms = {E, raw_planes, 0, n_elems, nullptr};
  PlanesGatherParams g = {};
  for (uint32_t p = 0; p < E; ++p) {
    g.streams[p] = h_stream_ptrs[p];
    g.stream_bytes[p] = h_stream_bytes[p];
    g.records[p] = forms.is_raw(p) ? nullptr : h_table_ptrs[p] + kSeekHeaderBytes;
  }
  g.codes = d_codes;
  g.n_elems = n_elems;
  g.n_blocks = blocks_for(n_elems);  // what seek_table_ok held every table's size against
  g.index = d_index;
  g.index_stride = index_stride;
  g.row_elems = row_elems;
  g.n_rows = n_rows;
  g.out = d_out;
  g.out_stride = out_stride;
  g.row_status = d_row_status;
  return queued(c, [&] { launch_decode_planes_gather(g, E, raw_planes, c->stream); });
}

// (no reference counterpart)  The same rows of a tensor in any mix of the three forms, against a base
// where there is one: the slots of the slot rule, the rank tables as images in device memory.
int ghf_decode_planes_gather_forms(ghf_ctx* c, const uint8_t* const* h_stream_ptrs, const size_t* h_stream_bytes, const ghf_code* d_codes,
                                   const ghf_seek_info* h_infos, const uint8_t* const* h_table_ptrs, const size_t* h_table_bytes,
                                   const ghf_sparse_rank_info* h_rank_infos, const uint8_t* const* h_rank_ptrs, const size_t* h_rank_bytes,
                                   const uint8_t* d_base, unsigned raw_planes, unsigned sparse_planes, size_t n_elems, uint32_t elem_bytes,
                                   const uint64_t* d_index, uint64_t index_stride, uint32_t row_elems, uint32_t n_rows, uint8_t* d_out,
                                   size_t out_stride, int32_t* d_row_status) {
  if (!c) return GHF_E_INVAL;
  const char* const who = "ghf_decode_planes_gather_forms";
  const std::string f = std::string(who) + ": ";
  const uint32_t E = elem_bytes;
  int rc = gather_args(c, who, h_stream_ptrs, h_stream_bytes, d_codes, h_infos, h_table_ptrs, h_table_bytes, raw_planes,
                       elem_bytes_ok(E) ? sparse_planes & ~raw_planes & ((1u << E) - 1u) : sparse_planes, n_elems, E, d_index, row_elems, d_out,
                       out_stride, d_row_status);
  if (rc) return rc;
  size_t n_vals[GHF_PLANES_MAX] = {};  // of the sparse planes: what their rank infos count, once those are checked
  const PlaneForms forms = {E, raw_planes, sparse_planes, n_elems, n_vals};
  if (!forms.sparse_planes_ok(false) || !forms.forms_ok(false))
    return fail(c, GHF_E_INVAL, (f + "the masks have bits below elem_bytes only and name no plane twice").c_str());
  if (sparse_planes && (!h_rank_infos || !h_rank_ptrs || !h_rank_bytes)) return fail(c, GHF_E_INVAL, (f + "sparse planes need their rank tables").c_str());
  for (uint32_t p = 0; p < E; ++p)
    if (forms.is_sparse(p) && (!h_rank_ptrs[p] || (reinterpret_cast<uintptr_t>(h_rank_ptrs[p]) & 7u) || h_rank_bytes[p] != ghf_sparse_rank_bytes(n_elems)))
      return fail(c, GHF_E_INVAL, (f + "a rank table is null, not 8-byte aligned or not ghf_sparse_rank_bytes(n_elems) long").c_str());
  for (uint32_t p = 0; p < E; ++p) {
    if (!forms.is_sparse(p)) continue;
    if (h_rank_infos[p].n != n_elems) return fail(c, GHF_E_INVAL, (f + "a rank table is not one of n_elems elements").c_str());
    if (h_rank_infos[p].version != kSparseRankVersion || h_rank_infos[p].n_blocks != rank_blocks_for(n_elems) || h_rank_infos[p].n_vals > n_elems)
      return fail(c, GHF_E_FORMAT, (f + "a rank info is not what ghf_sparse_rank_parse fills in").c_str());
    n_vals[p] = (size_t)h_rank_infos[p].n_vals;
  }
  for (uint32_t p = 0; p < E; ++p)
    if (forms.is_sparse(p) && h_infos[p].n_symbols != forms.symbols(p))
      return fail(c, GHF_E_INVAL, (f + "a mask stream does not have ghf_sparse_mask_bytes(n_elems) symbols").c_str());
  for (uint32_t p = 0; p < E; ++p) {
    const uint32_t j = E + p;
    if (!forms.is_sparse(p) || !forms.stored(j)) continue;  // the values slot of any other plane is ignored
    if (!h_stream_ptrs[j] || !aligned16(h_stream_ptrs[j]) || !h_table_ptrs[j] || !aligned16(h_table_ptrs[j]))
      return fail(c, GHF_E_INVAL, (f + "a stream or table pointer is null or not 16-byte aligned").c_str());
    if (h_infos[j].n_symbols != forms.symbols(j))
      return fail(c, GHF_E_INVAL, (f + "a values stream does not have the symbols its rank table counts").c_str());
    if ((rc = seek_table_ok(c, who, h_infos + j, h_table_ptrs[j], h_table_bytes[j]))) return rc;
  }
  if (n_rows == 0) return GHF_OK;
  PlanesGatherFormsParams g = {};
  for (uint32_t j = 0; j < 2 * E; ++j) {
    if (!forms.stored(j)) continue;
    g.streams[j] = h_stream_ptrs[j];
    g.stream_bytes[j] = h_stream_bytes[j];
    g.records[j] = forms.coded(j) ? h_table_ptrs[j] + kSeekHeaderBytes : nullptr;
  }
  for (uint32_t p = 0; p < E; ++p) {
    if (!forms.is_sparse(p)) continue;
    g.cum[p] = reinterpret_cast<const uint64_t*>(h_rank_ptrs[p] + kSparseRankHeaderBytes);
    g.n_vals[p] = n_vals[p];
  }
  g.codes = d_codes;
  g.base = d_base;
  g.n_elems = n_elems;
  g.index = d_index;
  g.index_stride = index_stride;
  g.row_elems = row_elems;
  g.n_rows = n_rows;
  g.out = d_out;
  g.out_stride = out_stride;
  g.row_status = d_row_status;
  return queued(c, [&] { launch_decode_planes_gather_forms(g, E, raw_planes, sparse_planes, c->stream); });
}

}  // extern "C"
