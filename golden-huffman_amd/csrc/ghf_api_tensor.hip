// golden-huffman_amd/csrc/ghf_api_tensor.hip -- the container calls of the C ABI (include/ghf_tensor.h):
// bound, pack, compress, workspace release, parse, open, close, describe, and the three thin decode drivers.  Host-side only, like ghf_api_planes.hip:
// argument checks, the layout of the host-known part, launches.  The planes themselves are compressed and decoded by the drivers
// of ghf_api_planes.hip, which this unit calls and does not restate.
#include <cstring>
#include <string>
#include <vector>

#include "ghf_ctx.h"

using namespace ghf;

namespace {

inline uint64_t pad16(uint64_t x) { return (x + 15u) & ~15ull; }
inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

// THE HOST-KNOWN PART of a container: the directory entries of the seek tables (by slot) and of the rank tables (by plane), in
// the order the format gives them -- the tables j ascending, then the ranks p ascending, from byte 768 -- and where the streams begin
struct FixedLayout {
  ghf_tensor_section table[kTensorSlots], rank[GHF_PLANES_MAX];
  uint64_t streams_off;
};
FixedLayout fixed_layout(const PlaneForms& forms) {
  FixedLayout L = {};
  const uint32_t E = forms.elem_bytes;
  uint64_t at = kTensorHeadBytes;
  for (uint32_t j = 0; j < 2 * E; ++j) {
    if (!forms.coded(j)) continue;
    L.table[j] = {at, (uint64_t)ghf_seek_bytes(forms.symbols(j))};
    at = pad16(at + L.table[j].bytes);
  }
  for (uint32_t p = 0; p < E; ++p) {
    if (!forms.is_sparse(p)) continue;
    L.rank[p] = {at, (uint64_t)ghf_sparse_rank_bytes(forms.n_elems)};
    at = pad16(at + L.rank[p].bytes);
  }
  L.streams_off = at;
  return L;
}

}  // namespace

// an opened container: what the decode drivers hand to the forms calls, built once
struct ghf_tensor {
  int device = 0;
  ghf_tensor_info info = {};
  const uint8_t* d_container = nullptr;
  size_t container_bytes = 0;
  ghf_code* d_codes = nullptr;  // DEVICE [2 * elem_bytes]: zero where a stream has no code or did not pass k_tensor_open
  const uint8_t* stream_ptrs[kTensorSlots] = {};
  size_t stream_bytes[kTensorSlots] = {};
  ghf_seek_info seek_infos[kTensorSlots] = {};
  const uint8_t* table_ptrs[kTensorSlots] = {};
  size_t table_bytes[kTensorSlots] = {};
  ghf_sparse_rank_info rank_infos[GHF_PLANES_MAX] = {};
  const uint8_t* rank_dev[GHF_PLANES_MAX] = {};   // the images in the container (the gather reads cum[] on the device)
  const uint8_t* rank_host[GHF_PLANES_MAX] = {};  // ... and on the host (the range call reads two entries here)
  size_t rank_bytes[GHF_PLANES_MAX] = {};
  size_t n_vals[GHF_PLANES_MAX] = {};
  std::vector<uint8_t> ranks;  // what rank_host points into
};

extern "C" {

size_t ghf_tensor_bound(size_t n_elems, uint32_t elem_bytes) {
  if (!elem_bytes_ok(elem_bytes) || n_elems > ((size_t)1 << 56)) return 0;
  const size_t E = elem_bytes;
  return kTensorHeadBytes + 2 * E * (size_t)pad16(ghf_seek_bytes(n_elems)) + E * (size_t)pad16(ghf_sparse_rank_bytes(n_elems)) +
         2 * E * ghf_planes_slot_bytes(n_elems);
}

int ghf_tensor_pack(ghf_ctx* c, const uint8_t* const* h_stream_ptrs, const uint64_t* d_stream_bytes, const ghf_index* h_indexes,
                    const uint8_t* const* h_rank_ptrs, unsigned raw_planes, unsigned sparse_planes, const size_t* h_n_vals, size_t n_elems,
                    uint32_t elem_bytes, unsigned flags, uint8_t* d_container, size_t cap, uint64_t* d_container_bytes) {
  if (!c || !h_stream_ptrs || !d_stream_bytes || !h_indexes || !h_n_vals || !d_container || !d_container_bytes) return GHF_E_INVAL;
  const std::string f = "ghf_tensor_pack: ";
  const uint32_t E = elem_bytes;
  if (!elem_bytes_ok(E)) return fail(c, GHF_E_INVAL, (f + "elem_bytes must be 2, 4 or 8").c_str());
  const PlaneForms forms = {E, raw_planes, sparse_planes, n_elems, h_n_vals};
  if (!forms.sparse_planes_ok(false))
    return fail(c, GHF_E_INVAL, (f + "sparse_planes has bits below elem_bytes only (the mask the compress call reported)").c_str());
  if (!forms.forms_ok(false))
    return fail(c, GHF_E_INVAL, (f + "raw_planes has bits below elem_bytes only, none of them a sparse plane's").c_str());
  if (flags & ~GHF_TENSOR_DELTA) return fail(c, GHF_E_INVAL, (f + "unknown flags").c_str());
  for (uint32_t p = 0; p < E; ++p)
    if (forms.is_sparse(p) && h_n_vals[p] > n_elems) return fail(c, GHF_E_INVAL, (f + "a plane has more values than elements").c_str());
  for (uint32_t j = 0; j < 2 * E; ++j)
    if (forms.stored(j) && (!h_stream_ptrs[j] || !aligned16(h_stream_ptrs[j])))
      return fail(c, GHF_E_INVAL, (f + "a stream pointer is null or not 16-byte aligned").c_str());
  if (!aligned16(d_container) || !aligned8(d_stream_bytes) || !aligned8(d_container_bytes))
    return fail(c, GHF_E_INVAL, (f + "d_container must be 16-byte, d_stream_bytes and d_container_bytes 8-byte aligned").c_str());
  if (sparse_planes && !h_rank_ptrs) return fail(c, GHF_E_INVAL, (f + "sparse planes need their rank tables").c_str());
  for (uint32_t p = 0; p < E; ++p)
    if (forms.is_sparse(p) && (!h_rank_ptrs[p] || !aligned8(h_rank_ptrs[p])))
      return fail(c, GHF_E_INVAL, (f + "a rank table is null or not 8-byte aligned").c_str());
  if (n_elems > (size_t)-1 / E - 255) return fail(c, GHF_E_INVAL, (f + "n_elems * elem_bytes overflows").c_str());
  for (uint32_t j = 0; j < 2 * E; ++j)
    if (forms.coded(j) && (h_indexes[j].n_symbols != forms.symbols(j) || !index_is_whole(&h_indexes[j])))
      return fail(c, GHF_E_INVAL, (f + "an index does not cover exactly the symbols of its stream").c_str());
  if (n_elems == 0) return fail(c, GHF_E_EMPTY, (f + "no elements").c_str());
  const FixedLayout L = fixed_layout(forms);
  if (cap < L.streams_off) return fail(c, GHF_E_CAP, (f + "cap below the head and the tables").c_str());
  GHF_HIP(c, hipSetDevice(c->device));
  // everything with a size the host knows goes straight into the container ...
  int rc;
  for (uint32_t j = 0; j < 2 * E; ++j)
    if (forms.coded(j) && (rc = ghf_seek_pack(c, &h_indexes[j], h_stream_ptrs[j], 0, d_container + L.table[j].offset, (size_t)L.table[j].bytes)))
      return rc;
  for (uint32_t p = 0; p < E; ++p)
    if (forms.is_sparse(p))
      GHF_HIP(c, hipMemcpyAsync(d_container + L.rank[p].offset, h_rank_ptrs[p], (size_t)L.rank[p].bytes, hipMemcpyDeviceToDevice, c->stream));
  // ... and one kernel places the streams, whose sizes only the device knows, and the head
  TensorPackParams P = {};
  uint64_t most = 0;  // the most bytes the stream region can have: what sizes the grid
  for (uint32_t j = 0; j < 2 * E; ++j) {
    if (!forms.stored(j)) continue;
    P.streams[j] = h_stream_ptrs[j];
    P.stored |= 1u << j;
    most += forms.coded(j) ? ghf_planes_slot_bytes(forms.symbols(j)) : pad16(n_elems);
  }
  P.stream_bytes = d_stream_bytes;
  P.elem_bytes = E;
  P.raw_planes = raw_planes;
  P.sparse_planes = sparse_planes;
  P.flags = flags;
  P.n_elems = n_elems;
  for (uint32_t p = 0; p < E; ++p) P.n_vals[p] = forms.is_sparse(p) ? h_n_vals[p] : 0;
  for (uint32_t j = 0; j < kTensorSlots; ++j) P.fixed_off[j] = L.table[j].offset, P.fixed_bytes[j] = L.table[j].bytes;
  for (uint32_t p = 0; p < GHF_PLANES_MAX; ++p) P.fixed_off[kTensorSlots + p] = L.rank[p].offset, P.fixed_bytes[kTensorSlots + p] = L.rank[p].bytes;
  P.streams_off = L.streams_off;
  P.out = d_container;
  P.cap = cap;
  P.out_bytes = d_container_bytes;
  P.status = c->d_status;
  const uint64_t groups = std::min<uint64_t>(kTensorPackGroups, std::max<uint64_t>(1, (most / 16 + 1023) / 1024));
  launch_tensor_pack(P, (uint32_t)groups, c->stream);
  GHF_HIP(c, hipGetLastError());
  return GHF_OK;
}

int ghf_compress_tensor(ghf_ctx* c, const uint8_t* d_in, const uint8_t* d_base, size_t n_elems, uint32_t elem_bytes, unsigned raw_planes,
                        unsigned sparse_planes, uint8_t* d_container, size_t cap, uint64_t* d_container_bytes) {
  if (!c || !d_in || !d_container || !d_container_bytes) return GHF_E_INVAL;
  const std::string f = "ghf_compress_tensor: ";
  const uint32_t E = elem_bytes;
  // what sizes the workspaces must be good before they are; the planes' driver repeats these among its own refusals
  if (!elem_bytes_ok(E)) return fail(c, GHF_E_INVAL, (f + "elem_bytes must be 2, 4 or 8").c_str());
  if (!aligned16(d_container) || !aligned8(d_container_bytes))
    return fail(c, GHF_E_INVAL, (f + "d_container must be 16-byte, d_container_bytes 8-byte aligned").c_str());
  if (n_elems > ((size_t)1 << 56)) return fail(c, GHF_E_INVAL, (f + "n_elems * elem_bytes overflows").c_str());
  if (n_elems == 0) return fail(c, GHF_E_EMPTY, (f + "no elements").c_str());
  GHF_HIP(c, hipSetDevice(c->device));
  const size_t slot_bytes = ghf_planes_slot_bytes(n_elems), rank_slot_bytes = (size_t)pad16(ghf_sparse_rank_bytes(n_elems));
  int rc = grow(c, c->tensor_slots, 2 * E * slot_bytes);
  if (!rc) rc = grow(c, c->tensor_ranks, E * rank_slot_bytes);
  if (!rc) rc = grow(c, c->tensor_sizes, kTensorSlots);
  if (rc) return rc;
  ghf_index idx[kTensorSlots];
  unsigned raw = 0, sparse = 0;
  size_t n_vals[GHF_PLANES_MAX] = {};
  if ((rc = compress_planes_forms(c, "ghf_compress_tensor", d_in, d_base, n_elems, E, raw_planes, sparse_planes, c->tensor_slots.p, slot_bytes,
                                  c->tensor_sizes.p, nullptr, idx, true, c->tensor_ranks.p, rank_slot_bytes, &raw, &sparse, n_vals)))
    return rc;
  const uint8_t *slots[kTensorSlots], *ranks[GHF_PLANES_MAX];
  for (uint32_t j = 0; j < 2 * E; ++j) slots[j] = c->tensor_slots.p + j * slot_bytes;
  for (uint32_t p = 0; p < E; ++p) ranks[p] = c->tensor_ranks.p + p * rank_slot_bytes;
  return ghf_tensor_pack(c, slots, c->tensor_sizes.p, idx, ranks, raw, sparse, n_vals, n_elems, E, d_base ? GHF_TENSOR_DELTA : 0u, d_container,
                         cap, d_container_bytes);
}

int ghf_tensor_workspace_release(ghf_ctx* c) {
  if (!c) return GHF_E_INVAL;
  GHF_HIP(c, hipSetDevice(c->device));
  GHF_HIP(c, hipStreamSynchronize(c->stream));  // a pack queued on the context may still read the slots
  release(c->tensor_slots);
  release(c->tensor_ranks);
  release(c->tensor_sizes);
  release(c->tensor_chunk_bit);
  release(c->tensor_seg_bit);
  return GHF_OK;
}

int ghf_tensor_parse(const uint8_t* h, size_t head_bytes, size_t container_bytes, ghf_tensor_info* info) {
  if (!h || !info) return GHF_E_INVAL;
  std::memset(info, 0, sizeof *info);
  if (head_bytes < kTensorHeadBytes || container_bytes < kTensorHeadBytes) return GHF_E_FORMAT;
  if (le64(h) != kTensorMagic || le32(h + 8) != kTensorVersion) return GHF_E_FORMAT;
  ghf_tensor_info t = {};
  t.version = kTensorVersion;
  t.elem_bytes = le32(h + 12);
  t.n_elems = le64(h + 16);
  t.raw_planes = le32(h + 24);
  t.sparse_planes = le32(h + 28);
  t.flags = le32(h + 32);
  t.total_bytes = le64(h + 40);
  const uint32_t E = t.elem_bytes;
  if (!elem_bytes_ok(E)) return GHF_E_FORMAT;
  if ((t.raw_planes >> E) || (t.sparse_planes >> E) || (t.raw_planes & t.sparse_planes) || (t.flags & ~GHF_TENSOR_DELTA)) return GHF_E_FORMAT;
  if (le32(h + 36) || le64(h + 48) || le64(h + 56)) return GHF_E_FORMAT;  // the reserved bytes
  if (t.n_elems == 0 || t.n_elems > ((uint64_t)1 << 56)) return GHF_E_FORMAT;
  size_t n_vals[GHF_PLANES_MAX] = {};
  for (uint32_t p = 0; p < GHF_PLANES_MAX; ++p) {
    t.n_vals[p] = le64(h + 64 + 8 * p);
    const bool sparse = p < E && ((t.sparse_planes >> p) & 1u);
    if (sparse ? t.n_vals[p] > t.n_elems : t.n_vals[p] != 0) return GHF_E_FORMAT;
    n_vals[p] = (size_t)t.n_vals[p];
  }
  for (uint32_t k = 0; k < GHF_TENSOR_DIR_ENTRIES; ++k) t.dir[k] = {le64(h + 128 + 16 * k), le64(h + 136 + 16 * k)};
  const PlaneForms forms = {E, t.raw_planes, t.sparse_planes, (size_t)t.n_elems, n_vals};
  // the sections in the order of the payload; `at` is the least offset the next one may have
  uint64_t at = kTensorHeadBytes;
  const auto section = [&](const ghf_tensor_section& s, bool present, uint64_t want_bytes /* 0: whatever it says */) {
    if (!present) return s.offset == 0 && s.bytes == 0;
    if ((s.offset & 15u) || s.offset < at || s.bytes == 0 || s.offset > container_bytes || s.bytes > container_bytes - s.offset) return false;
    if (want_bytes && s.bytes != want_bytes) return false;
    at = pad16(s.offset + s.bytes);
    return true;
  };
  for (uint32_t j = 0; j < kTensorSlots; ++j)
    if (!section(t.dir[kTensorSlots + j], j < 2 * E && forms.coded(j), j < 2 * E ? ghf_seek_bytes(forms.symbols(j)) : 0)) return GHF_E_FORMAT;
  for (uint32_t p = 0; p < GHF_PLANES_MAX; ++p)
    if (!section(t.dir[2 * kTensorSlots + p], p < E && forms.is_sparse(p), ghf_sparse_rank_bytes((size_t)t.n_elems))) return GHF_E_FORMAT;
  for (uint32_t j = 0; j < kTensorSlots; ++j)
    if (!section(t.dir[j], j < 2 * E && forms.stored(j), j < E && forms.is_raw(j) ? t.n_elems : 0)) return GHF_E_FORMAT;
  if (t.total_bytes != at || t.total_bytes > container_bytes) return GHF_E_FORMAT;
  *info = t;
  return GHF_OK;
}

int ghf_tensor_open(ghf_ctx* c, const uint8_t* h_head, size_t head_bytes, const uint8_t* d_container, size_t container_bytes,
                    ghf_tensor** out) {
  if (out) *out = nullptr;
  if (!c || !d_container || !out) return GHF_E_INVAL;
  const std::string f = "ghf_tensor_open: ";
  if (!aligned16(d_container)) return fail(c, GHF_E_INVAL, (f + "d_container must be 16-byte aligned").c_str());
  uint8_t fetched[kTensorHeadBytes];
  if (!h_head) {  // the head from the container itself: the one wait a caller without it pays
    if (container_bytes < kTensorHeadBytes) return fail(c, GHF_E_FORMAT, (f + "the container is shorter than its head").c_str());
    GHF_HIP(c, hipSetDevice(c->device));
    GHF_HIP(c, hipMemcpyAsync(fetched, d_container, kTensorHeadBytes, hipMemcpyDeviceToHost, c->stream));
    GHF_HIP(c, hipStreamSynchronize(c->stream));
    h_head = fetched;
    head_bytes = kTensorHeadBytes;
  }
  ghf_tensor_info info;
  if (ghf_tensor_parse(h_head, head_bytes, container_bytes, &info)) return fail(c, GHF_E_FORMAT, (f + "not the head of a tensor container of this size").c_str());
  GHF_HIP(c, hipSetDevice(c->device));
  ghf_tensor* t = new ghf_tensor;
  t->device = c->device;
  t->info = info;
  t->d_container = d_container;
  t->container_bytes = container_bytes;
  const uint32_t E = info.elem_bytes;
  for (uint32_t p = 0; p < E; ++p) t->n_vals[p] = (size_t)info.n_vals[p];
  const PlaneForms forms = {E, info.raw_planes, info.sparse_planes, (size_t)info.n_elems, t->n_vals};
  hipError_t e = hipMalloc(&t->d_codes, 2 * E * sizeof(ghf_code));
  if (e == hipSuccess) e = hipMemsetAsync(t->d_codes, 0, 2 * E * sizeof(ghf_code), c->stream);
  if (e != hipSuccess) {
    if (t->d_codes) (void)hipFree(t->d_codes);
    delete t;
    return fail(c, GHF_E_HIP, (f + "the codes").c_str(), e);
  }
  TensorOpenParams P = {};
  P.container = d_container;
  P.n_elems = info.n_elems;
  P.codes = t->d_codes;
  P.status = c->d_status;
  size_t ranks_bytes = 0;
  for (uint32_t p = 0; p < E; ++p) {
    if (!forms.is_sparse(p)) continue;
    const ghf_tensor_section& r = info.dir[2 * kTensorSlots + p];
    t->rank_dev[p] = d_container + r.offset;
    t->rank_bytes[p] = (size_t)r.bytes;
    ranks_bytes += (size_t)r.bytes;
  }
  for (uint32_t j = 0; j < 2 * E; ++j) {
    if (!forms.stored(j)) continue;
    t->stream_ptrs[j] = d_container + info.dir[j].offset;
    t->stream_bytes[j] = (size_t)info.dir[j].bytes;
    if (!forms.coded(j)) continue;
    const ghf_tensor_section& tab = info.dir[kTensorSlots + j];
    t->table_ptrs[j] = d_container + tab.offset;
    t->table_bytes[j] = (size_t)tab.bytes;
    t->seek_infos[j] = {forms.symbols(j), blocks_for(forms.symbols(j)), 0u, kSeekVersion};
    const uint32_t b = P.n_streams++;
    P.slot[b] = j;
    P.stream_off[b] = info.dir[j].offset;
    P.stream_bytes[b] = info.dir[j].bytes;
    P.table_off[b] = tab.offset;
    P.symbols[b] = forms.symbols(j);
    if (j < E && forms.is_sparse(j)) {
      P.rank_off[b] = info.dir[2 * kTensorSlots + j].offset;
      P.rank_n_vals[b] = info.n_vals[j];
    }
  }
  launch_tensor_open(P, c->stream);
  e = hipGetLastError();
  // the rank tables on the host, for the range call: the one wait of an open, and only with a sparse plane
  if (e == hipSuccess && ranks_bytes) {
    t->ranks.resize(ranks_bytes);
    size_t at = 0;
    for (uint32_t p = 0; p < E && e == hipSuccess; ++p) {
      if (!forms.is_sparse(p)) continue;
      t->rank_host[p] = t->ranks.data() + at;
      e = hipMemcpyAsync(t->ranks.data() + at, t->rank_dev[p], t->rank_bytes[p], hipMemcpyDeviceToHost, c->stream);
      at += t->rank_bytes[p];
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  }
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(c->stream);
    (void)ghf_tensor_close(t);
    return fail(c, GHF_E_HIP, (f + "launch").c_str(), e);
  }
  for (uint32_t p = 0; p < E; ++p) {
    if (!forms.is_sparse(p)) continue;
    if (ghf_sparse_rank_parse(t->rank_host[p], t->rank_bytes[p], &t->rank_infos[p]) || t->rank_infos[p].n != info.n_elems ||
        t->rank_infos[p].n_vals != info.n_vals[p]) {
      (void)ghf_tensor_close(t);  // the stream is idle: the wait above
      return fail(c, GHF_E_FORMAT, (f + "a rank table is not the one the head describes").c_str());
    }
  }
  *out = t;
  return GHF_OK;
}

int ghf_tensor_close(ghf_tensor* t) {
  if (!t) return GHF_OK;
  (void)hipSetDevice(t->device);
  if (t->d_codes) (void)hipFree(t->d_codes);
  delete t;
  return GHF_OK;
}

int ghf_tensor_describe(const ghf_tensor* t, ghf_tensor_info* info) {
  if (!t || !info) return GHF_E_INVAL;
  *info = t->info;
  return GHF_OK;
}

// a container of new ^ base is decoded against the base and no other container is
static int base_matches_flag(ghf_ctx* c, const char* who, const ghf_tensor* t, const uint8_t* d_base) {
  if (((t->info.flags & GHF_TENSOR_DELTA) != 0) == (d_base != nullptr)) return GHF_OK;
  return fail(c, GHF_E_INVAL, (std::string(who) + (d_base ? ": the container is not one of new ^ base: d_base must be NULL"
                                                          : ": the container holds new ^ base (GHF_TENSOR_DELTA): d_base is required")).c_str());
}

int ghf_tensor_decode_range(ghf_ctx* c, const ghf_tensor* t, const uint8_t* d_base, uint64_t first, uint64_t count, uint8_t* d_out,
                            size_t cap) {
  if (!c || !t) return GHF_E_INVAL;
  const int rc = base_matches_flag(c, "ghf_tensor_decode_range", t, d_base);
  if (rc) return rc;
  const ghf_tensor_info& i = t->info;
  return ghf_decode_planes_forms_range(c, t->stream_ptrs, t->stream_bytes, t->d_codes, nullptr, t->seek_infos, t->table_ptrs, t->table_bytes,
                                       t->rank_infos, t->rank_host, d_base, i.raw_planes, i.sparse_planes, (size_t)i.n_elems, i.elem_bytes,
                                       first, count, d_out, cap);
}

int ghf_tensor_decode(ghf_ctx* c, const ghf_tensor* t, const uint8_t* d_base, uint8_t* d_out, size_t cap, uint64_t* d_out_bytes) {
  if (!c || !t) return GHF_E_INVAL;
  int rc = base_matches_flag(c, "ghf_tensor_decode", t, d_base);
  if (rc) return rc;
  if (!aligned8(d_out_bytes)) return fail(c, GHF_E_INVAL, "ghf_tensor_decode: d_out_bytes must be 8-byte aligned");
  const ghf_tensor_info& i = t->info;
  if ((rc = ghf_decode_planes_forms_range(c, t->stream_ptrs, t->stream_bytes, t->d_codes, nullptr, t->seek_infos, t->table_ptrs, t->table_bytes,
                                          t->rank_infos, t->rank_host, d_base, i.raw_planes, i.sparse_planes, (size_t)i.n_elems, i.elem_bytes, 0,
                                          i.n_elems, d_out, cap)))
    return rc;
  if (!d_out_bytes) return GHF_OK;
  // behind a latched status the decode stored nothing, and the size says nothing either
  return queued(c, [&] { launch_tensor_store_size(d_out_bytes, i.n_elems * i.elem_bytes, c->d_status, c->stream); });
}

int ghf_tensor_gather(ghf_ctx* c, const ghf_tensor* t, const uint8_t* d_base, const uint64_t* d_index, uint64_t index_stride,
                      uint32_t row_elems, uint32_t n_rows, uint8_t* d_out, size_t out_stride, int32_t* d_row_status) {
  if (!c || !t) return GHF_E_INVAL;
  const int rc = base_matches_flag(c, "ghf_tensor_gather", t, d_base);
  if (rc) return rc;
  const ghf_tensor_info& i = t->info;
  return ghf_decode_planes_gather_forms(c, t->stream_ptrs, t->stream_bytes, t->d_codes, t->seek_infos, t->table_ptrs, t->table_bytes,
                                        t->rank_infos, t->rank_dev, t->rank_bytes, d_base, i.raw_planes, i.sparse_planes, (size_t)i.n_elems,
                                        i.elem_bytes, d_index, index_stride, row_elems, n_rows, d_out, out_stride, d_row_status);
}

}  // extern "C"
