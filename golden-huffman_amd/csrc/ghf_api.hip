// golden-huffman_amd/csrc/ghf_api.hip -- the C ABI of include/ghf.h on top of the gfx950 kernels.
// Host-side only: argument checks, workspace, launches.  No compute happens on the CPU here except
// ghf_parse_header (a <= 1.3 KiB header; SURVEY 8 row a7 keeps it on the host).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>

#include "ghf_code_rules.h"
#include "ghf_ctx.h"

using namespace ghf;

namespace {

thread_local std::string g_create_err;  // ghf_last_error(NULL): why ghf_ctx_create failed

int ensure_ws(ghf_ctx* c, size_t nchunks) {
  bool new_off = false, new_hist = false;
  int rc = grow(c, c->chunk_off, nchunks + 1, 1024, &new_off);
  if (!rc) rc = grow(c, c->chunk_hist, nchunks * 256, 1024 * 256, &new_hist);
  if (new_off) c->plan.forget();
  if (new_hist) c->hist.forget();
  return rc;
}

}  // namespace

// ---- a range of a seekable stream: what ghf_ctx.h declares for this unit and ghf_api_planes.hip -------------------------
namespace ghf {

int seek_table_ok(ghf_ctx* c, const char* who, const ghf_seek_info* info, const uint8_t* d_table, size_t table_bytes) {
  const std::string f = std::string(who) + ": ";
  if (!aligned16(d_table)) return fail(c, GHF_E_INVAL, (f + "d_table must be 16-byte aligned").c_str());
  if (info->version != kSeekVersion || (info->flags & ~(uint32_t)GHF_INDEX_NO_END_MARK) || info->n_blocks != blocks_for(info->n_symbols) ||
      info->n_blocks >= kDecMaxGroups || table_bytes != ghf_seek_bytes(info->n_symbols))
    return fail(c, GHF_E_FORMAT, (f + "the seek table does not have the size its header implies").c_str());
  return GHF_OK;
}

SeekExpandParams seek_expand_params(ghf_ctx* c, const ghf_seek_info* info, const uint8_t* d_table, const uint8_t* d_stream,
                                    size_t stream_bytes, const DecTables* dt, uint64_t g0, uint64_t g1, uint64_t* chunk_bit,
                                    uint32_t* seg_bit) {
  SeekExpandParams p = {};
  p.records = d_table + kSeekHeaderBytes;
  p.stream = d_stream;
  p.stream_bytes = stream_bytes;
  p.dt = dt;
  p.n_symbols = info->n_symbols;
  p.n_blocks = info->n_blocks;
  p.g0 = g0;
  p.g1 = g1;
  p.chunk_bit = chunk_bit;
  p.seg_bit = seg_bit;
  p.status = c->d_status;
  return p;
}

DecParams range_decode_params(ghf_ctx* c, const uint8_t* d_stream, size_t stream_bytes, DecTables* dt, const uint64_t* chunk_bit,
                              const uint32_t* seg_bit, uint64_t g, uint64_t end, uint64_t n, uint32_t index_flags, uint8_t* out) {
  DecParams p = {};
  p.stream = d_stream;
  p.stream_bytes = stream_bytes;
  p.dt = dt;
  p.chunk_bit = chunk_bit;
  p.seg_bit = seg_bit;
  p.n_symbols = end - g * kBlockSymbols;
  p.n_segs = segs_for(p.n_symbols);
  p.no_end_mark = (end == n && !(index_flags & GHF_INDEX_NO_END_MARK)) ? 0u : 1u;
  p.out = out;
  p.out_bytes = nullptr;
  p.status = c->d_status;
  return p;
}

}  // namespace ghf

extern "C" {

int ghf_version(void) { return 210; }  // 2.1: events, ghf_histogram_add, GHF_EMPTY_OK, table validation

const char* ghf_status_string(int s) {
  switch (s) {
    case GHF_OK: return "ok";
    case GHF_E_INVAL: return "invalid argument";
    case GHF_E_HIP: return "HIP runtime error / no device";
    case GHF_E_EMPTY: return "empty input (undefined in the reference)";
    case GHF_E_CODELEN: return "code longer than 32 bits (reference limit)";
    case GHF_E_CAP: return "output capacity too small";
    case GHF_E_FORMAT: return "not a .crs2 / .crs header";
    case GHF_E_CORRUPT: return "corrupt stream";
    case GHF_E_NOMEM: return "out of memory";
    case GHF_E_SINGLE: return "one distinct byte value (.crs: undefined in the reference)";
    case GHF_E_NOCODE: return "a byte value without a code in the shared code";
    default: return "unknown status";
  }
}

int ghf_ctx_create(int device, ghf_ctx** out) {
  if (!out) return GHF_E_INVAL;
  *out = nullptr;
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0) {  // no CPU fallback, by design
    g_create_err = std::string("hipGetDeviceCount: ") + (e != hipSuccess ? hipGetErrorString(e) : "no device");
    return GHF_E_HIP;
  }
  if (device < 0 || device >= ndev) return GHF_E_INVAL;
  ghf_ctx* c = new (std::nothrow) ghf_ctx();
  if (!c) return GHF_E_NOMEM;
  c->device = device;
  const char* what = "hipSetDevice";
  e = hipSetDevice(device);
#define GHF_STEP(call)      \
  if (e == hipSuccess) {    \
    what = #call;           \
    e = (call);             \
  }
  GHF_STEP(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
  GHF_STEP(hipMalloc(&c->d_status, sizeof(int)));
  GHF_STEP(hipHostMalloc(&c->h_status, sizeof(int), hipHostMallocDefault));
  GHF_STEP(hipMalloc(&c->d_hist, GHF_NSYM * sizeof(uint64_t)));
  GHF_STEP(hipMalloc(&c->d_hist_acc, kHistAccWords * sizeof(uint64_t)));
  GHF_STEP(hipMemset(c->d_hist_acc, 0, kHistAccWords * sizeof(uint64_t)));
  GHF_STEP(hipMalloc(&c->d_code, sizeof(ghf_code)));
  GHF_STEP(hipMalloc(&c->d_tree, sizeof(ghf_tree)));
  GHF_STEP(hipMalloc(&c->d_dt, sizeof(DecTables)));
  GHF_STEP(hipMalloc(&c->d, sizeof(Scalars)));
  GHF_STEP(hipHostMalloc(&c->h, sizeof(Scalars), hipHostMallocDefault));
  GHF_STEP(hipMalloc(&c->d_planes_hist_acc, kPlanesHistAccWords * sizeof(uint64_t)));
  GHF_STEP(hipMemset(c->d_planes_hist_acc, 0, kPlanesHistAccWords * sizeof(uint64_t)));
  GHF_STEP(hipMalloc(&c->d_planes_hists, ((size_t)GHF_PLANES_MAX * GHF_NSYM + GHF_PLANES_MAX) * sizeof(uint64_t)));
  GHF_STEP(hipMalloc(&c->d_sparse_counts, kSparseGroups * sizeof(uint64_t)));
  GHF_STEP(hipMalloc(&c->d_sparse_offs, kSparseOffWords * sizeof(uint64_t)));
  GHF_STEP(hipMemset(c->d_status, 0, sizeof(int)));
#undef GHF_STEP
  if (e != hipSuccess) {
    g_create_err = std::string(what) + ": " + hipGetErrorString(e);
    ghf_ctx_destroy(c);
    return GHF_E_HIP;
  }
  c->stream = c->own_stream;
  *out = c;
  return GHF_OK;
}

int ghf_ctx_destroy(ghf_ctx* c) {
  if (!c) return GHF_OK;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->d_status) (void)hipFree(c->d_status);
  if (c->h_status) (void)hipHostFree(c->h_status);
  if (c->d_hist) (void)hipFree(c->d_hist);
  if (c->d_hist_acc) (void)hipFree(c->d_hist_acc);
  if (c->d_code) (void)hipFree(c->d_code);
  if (c->d_tree) (void)hipFree(c->d_tree);
  if (c->d_dt) (void)hipFree(c->d_dt);
  if (c->d_planes_hist_acc) (void)hipFree(c->d_planes_hist_acc);
  if (c->d_planes_hists) (void)hipFree(c->d_planes_hists);
  if (c->d_sparse_counts) (void)hipFree(c->d_sparse_counts);
  if (c->d_sparse_offs) (void)hipFree(c->d_sparse_offs);
  if (c->d) (void)hipFree(c->d);
  if (c->h) (void)hipHostFree(c->h);
  release(c->chunk_hist);
  release(c->chunk_off);
  release(c->totals);
  release(c->sync);
  release(c->seg_bit);
  release(c->seg_abs);
  release(c->chunk_bit);
  release(c->range_seg);
  release(c->range_chunk);
  release(c->range_dt);
  release(c->batch_codes);
  release(c->planes);
  release(c->sparse);
  release(c->tensor_slots);
  release(c->tensor_ranks);
  release(c->tensor_sizes);
  release(c->tensor_chunk_bit);
  release(c->tensor_seg_bit);
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  delete c;
  return GHF_OK;
}

int ghf_ctx_set_stream(ghf_ctx* c, void* hip_stream) {
  if (!c) return GHF_E_INVAL;
  c->stream = reinterpret_cast<hipStream_t>(hip_stream);  // NULL is HIP's default (null) stream
  return GHF_OK;
}

int ghf_sync(ghf_ctx* c) {
  if (!c) return GHF_E_INVAL;
  GHF_HIP(c, hipSetDevice(c->device));
  GHF_HIP(c, hipMemcpyAsync(c->h_status, c->d_status, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  GHF_HIP(c, hipStreamSynchronize(c->stream));
  const int s = *c->h_status;
  if (s != GHF_OK) c->err = ghf_status_string(s);
  return s;
}

int ghf_status(ghf_ctx* c) { return ghf_sync(c); }

int ghf_clear_status(ghf_ctx* c) {
  if (!c) return GHF_E_INVAL;
  GHF_HIP(c, hipSetDevice(c->device));
  GHF_HIP(c, hipMemsetAsync(c->d_status, 0, sizeof(int), c->stream));
  GHF_HIP(c, hipMemsetAsync(c->d_hist_acc, 0, kHistAccWords * sizeof(uint64_t), c->stream));  // in case a launch died half-way
  c->err.clear();
  return GHF_OK;
}

const char* ghf_last_error(ghf_ctx* c) { return c ? c->err.c_str() : g_create_err.c_str(); }

// ---------------------------------------------------------------------------------------------- memory
int ghf_device_alloc(ghf_ctx* c, size_t bytes, void** d_ptr) {
  if (!c || !d_ptr) return GHF_E_INVAL;
  GHF_HIP(c, hipSetDevice(c->device));
  GHF_HIP(c, hipMalloc(d_ptr, bytes ? bytes : 16));
  return GHF_OK;
}
int ghf_device_free(ghf_ctx* c, void* d_ptr) {
  if (!c) return GHF_E_INVAL;
  if (d_ptr) {
    GHF_HIP(c, hipSetDevice(c->device));
    GHF_HIP(c, hipStreamSynchronize(c->stream));
    GHF_HIP(c, hipFree(d_ptr));
  }
  return GHF_OK;
}
int ghf_host_alloc(ghf_ctx* c, size_t bytes, void** h_ptr) {
  if (!c || !h_ptr) return GHF_E_INVAL;
  GHF_HIP(c, hipSetDevice(c->device));
  GHF_HIP(c, hipHostMalloc(h_ptr, bytes ? bytes : 16, hipHostMallocDefault));
  return GHF_OK;
}
int ghf_host_free(ghf_ctx* c, void* h_ptr) {
  if (!c) return GHF_E_INVAL;
  if (h_ptr) GHF_HIP(c, hipHostFree(h_ptr));
  return GHF_OK;
}
int ghf_copy_h2d(ghf_ctx* c, void* d_dst, const void* h_src, size_t bytes) {
  if (!c || (bytes && (!d_dst || !h_src))) return GHF_E_INVAL;
  GHF_HIP(c, hipSetDevice(c->device));
  if (bytes) GHF_HIP(c, hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, c->stream));
  return GHF_OK;
}
int ghf_copy_d2h(ghf_ctx* c, void* h_dst, const void* d_src, size_t bytes) {
  if (!c || (bytes && (!h_dst || !d_src))) return GHF_E_INVAL;
  GHF_HIP(c, hipSetDevice(c->device));
  if (bytes) GHF_HIP(c, hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, c->stream));
  return GHF_OK;
}
int ghf_copy_d2d(ghf_ctx* c, void* d_dst, const void* d_src, size_t bytes, int non_temporal) {
  if (!c || (bytes && (!d_dst || !d_src))) return GHF_E_INVAL;
  if (!aligned16(d_dst) || !aligned16(d_src)) return fail(c, GHF_E_INVAL, "ghf_copy_d2d: 16-byte aligned pointers");
  GHF_HIP(c, hipSetDevice(c->device));
  if (bytes) launch_stream_copy(static_cast<const uint8_t*>(d_src), static_cast<uint8_t*>(d_dst), bytes, non_temporal != 0, c->stream);
  return GHF_OK;
}
int ghf_memset_d(ghf_ctx* c, void* d_dst, int value, size_t bytes) {
  if (!c || (bytes && !d_dst)) return GHF_E_INVAL;
  GHF_HIP(c, hipSetDevice(c->device));
  if (bytes) GHF_HIP(c, hipMemsetAsync(d_dst, value, bytes, c->stream));
  return GHF_OK;
}

// ---------------------------------------------------------------------------------------------- events
struct ghf_event {
  int device = 0;
  hipEvent_t ev = nullptr;
};
int ghf_event_create(ghf_ctx* c, ghf_event** out) {
  if (!c || !out) return GHF_E_INVAL;
  GHF_HIP(c, hipSetDevice(c->device));
  ghf_event* e = new (std::nothrow) ghf_event;
  if (!e) return fail(c, GHF_E_HIP, "out of host memory");
  e->device = c->device;
  const hipError_t rc = hipEventCreateWithFlags(&e->ev, hipEventDisableTiming);
  if (rc != hipSuccess) {
    delete e;
    return fail(c, GHF_E_HIP, "hipEventCreateWithFlags", rc);
  }
  *out = e;
  return GHF_OK;
}
int ghf_event_destroy(ghf_event* e) {
  if (!e) return GHF_OK;
  (void)hipSetDevice(e->device);
  if (e->ev) (void)hipEventDestroy(e->ev);
  delete e;
  return GHF_OK;
}
int ghf_event_record(ghf_ctx* c, ghf_event* e) {
  if (!c || !e) return GHF_E_INVAL;
  GHF_HIP(c, hipSetDevice(c->device));
  GHF_HIP(c, hipEventRecord(e->ev, c->stream));
  return GHF_OK;
}
int ghf_event_wait(ghf_ctx* c, ghf_event* e) {
  if (!c || !e) return GHF_E_INVAL;
  GHF_HIP(c, hipSetDevice(c->device));
  GHF_HIP(c, hipStreamWaitEvent(c->stream, e->ev, 0));
  return GHF_OK;
}
int ghf_event_sync(ghf_event* e) {
  if (!e) return GHF_E_INVAL;
  if (hipSetDevice(e->device) != hipSuccess) return GHF_E_HIP;
  return hipEventSynchronize(e->ev) == hipSuccess ? GHF_OK : GHF_E_HIP;
}

// ---------------------------------------------------------------------------------------------- encode
uint32_t ghf_chunk_symbols(size_t n) { return chunk_symbols_for(n); }
size_t ghf_header_bytes(int max_len) { return header_bytes_for((size_t)max_len); }

size_t ghf_compress_bound(size_t n) {
  // header (max_len <= 32) + 9 bits per symbol (a 257-symbol Huffman code never loses to the 9-bit
  // fixed-length code) + end mark, rounded up to whole 16-byte units + one spare unit
  const size_t bits = 9 * (n + 1);
  size_t b = header_bytes_for(32) + (bits + 7) / 8;
  return ((b + 15) & ~(size_t)15) + 16;
}

static int histogram(ghf_ctx* c, const uint8_t* d_in, size_t n, uint64_t* d_hist, bool add) {
  if (!c || !d_hist || (n && !d_in)) return GHF_E_INVAL;
  GHF_HIP(c, hipSetDevice(c->device));
  const uint32_t cl = chunk_symbols_for(n);
  const size_t nchunks = (size_t)chunk_count_for(n);
  int rc = ensure_ws(c, nchunks);
  if (rc) return rc;
  launch_histogram(d_in, n, cl, (uint32_t)nchunks, c->chunk_hist.p, d_hist, c->d_hist_acc, add, c->stream);
  GHF_HIP(c, hipGetLastError());
  if (add) c->hist.forget();  // a piece's buffer is refilled before anything is planned: nothing to keep
  else c->hist = {d_in, n, cl};
  return GHF_OK;
}
int ghf_histogram(ghf_ctx* c, const uint8_t* d_in, size_t n, uint64_t* d_hist) { return histogram(c, d_in, n, d_hist, false); }
int ghf_histogram_add(ghf_ctx* c, const uint8_t* d_in, size_t n, uint64_t* d_hist) { return histogram(c, d_in, n, d_hist, true); }

int ghf_build_code_ex(ghf_ctx* c, const uint64_t* d_hist, ghf_code* d_code, unsigned flags) {
  if (!c || !d_hist || !d_code || (flags & ~(unsigned)(GHF_CODE_LIMIT | GHF_EMPTY_OK))) return GHF_E_INVAL;
  GHF_HIP(c, hipSetDevice(c->device));
  launch_build_code(d_hist, d_code, c->d_status, flags, c->stream);
  GHF_HIP(c, hipGetLastError());
  if (c->plan.code == d_code) c->plan.forget();  // tables changed: any cached plan is stale
  if (c->prepared.describes(d_code)) c->prepared.forget();
  return GHF_OK;
}

int ghf_build_code(ghf_ctx* c, const uint64_t* d_hist, ghf_code* d_code) { return ghf_build_code_ex(c, d_hist, d_code, 0); }

// n_codes exact builds in one launch: for the plane batches (ghf_api_batch.hip) and the staged plane calls (ghf_api_planes.hip)
int ghf_build_codes(ghf_ctx* c, const uint64_t* d_hists, uint32_t n_codes, ghf_code* d_codes, unsigned flags) {
  if (!c || !d_hists || !d_codes || n_codes == 0 || n_codes > GHF_PLANES_MAX || (flags & ~(unsigned)(GHF_CODE_LIMIT | GHF_EMPTY_OK)))
    return GHF_E_INVAL;
  GHF_HIP(c, hipSetDevice(c->device));
  launch_build_codes(d_hists, n_codes, d_codes, c->d_status, flags, c->stream);
  GHF_HIP(c, hipGetLastError());
  for (uint32_t k = 0; k < n_codes; ++k) {  // as ghf_build_code_ex: the tables changed, what was derived from them is stale
    if (c->plan.code == d_codes + k) c->plan.forget();
    if (c->prepared.describes(d_codes + k)) c->prepared.forget();
  }
  return GHF_OK;
}

int ghf_write_header(ghf_ctx* c, const ghf_code* d_code, uint8_t* d_out, size_t cap) {
  if (!c || !d_code || !d_out || (reinterpret_cast<uintptr_t>(d_out) & 3u)) return GHF_E_INVAL;
  GHF_HIP(c, hipSetDevice(c->device));
  launch_write_header(d_code, d_out, cap, c->d_status, c->stream);
  GHF_HIP(c, hipGetLastError());
  return GHF_OK;
}

int ghf_encode_plan(ghf_ctx* c, const uint8_t* d_in, size_t n, const ghf_code* d_code, uint64_t* d_total_bits) {
  if (!c || !d_code || (n && !d_in)) return GHF_E_INVAL;
  GHF_HIP(c, hipSetDevice(c->device));
  const uint32_t cl = chunk_symbols_for(n);
  const size_t nchunks = (size_t)chunk_count_for(n);
  int rc = ensure_ws(c, nchunks);
  if (rc) return rc;
  const bool have_hist = c->hist.describes(d_in, n, cl) && n != 0;
  launch_plan(d_in, n, cl, (uint32_t)nchunks, have_hist ? c->chunk_hist.p : nullptr, d_code, c->chunk_off.p,
              d_total_bits ? d_total_bits : &c->d->total_bits, c->stream);
  GHF_HIP(c, hipGetLastError());
  c->plan = {d_in, n, d_code};
  return GHF_OK;
}

int ghf_encode_emit(ghf_ctx* c, const uint8_t* d_in, size_t n, const ghf_code* d_code, const uint64_t* d_start_bit,
                    int flags, uint8_t* d_out, size_t cap, const ghf_index* index, uint64_t* d_end) {
  if (!c || !d_code || !d_out || (n && !d_in)) return GHF_E_INVAL;
  if (!aligned16(d_out)) return fail(c, GHF_E_INVAL, "d_out must be 16-byte aligned");
  if ((flags & GHF_EMIT_HEADER) && (flags & GHF_EMIT_REBASE))
    return fail(c, GHF_E_INVAL, "GHF_EMIT_HEADER is for the buffer that starts at stream byte 0 (rank 0 / single GPU)");
  if (!c->plan.describes(d_in, n, d_code))
    return fail(c, GHF_E_INVAL, "ghf_encode_emit: call ghf_encode_plan on the same (d_in, n, d_code) first");
  GHF_HIP(c, hipSetDevice(c->device));
  const uint32_t cl = chunk_symbols_for(n);
  const size_t nchunks = (size_t)chunk_count_for(n);
  if (index && (index->n_symbols != n || !index_has_arrays(index)))
    return fail(c, GHF_E_INVAL, "ghf_encode_emit: index does not match n (use ghf_index_alloc)");
  EmitParams p;
  p.in = d_in;
  p.n = n;
  p.code = d_code;
  p.chunk_off = c->chunk_off.p;
  p.d_start_bit = d_start_bit;
  p.out = d_out;
  p.cap = cap;
  p.chunk = cl;
  p.nchunks = (uint32_t)nchunks;
  p.chunk_bit = index ? index->d_chunk_bit : nullptr;
  p.seg_bit = index ? index->d_seg_bit : nullptr;
  p.flags = flags;
  p.status = c->d_status;
  p.d_end = d_end;
  launch_emit(p, c->stream);
  GHF_HIP(c, hipGetLastError());
  return GHF_OK;
}

int ghf_shard_start_bit(ghf_ctx* c, const ghf_code* d_code, const uint64_t* d_totals, int world, int rank,
                        uint64_t* d_start_bit) {
  if (!c || !d_code || !d_totals || !d_start_bit || world < 1 || rank < 0 || rank >= world) return GHF_E_INVAL;
  GHF_HIP(c, hipSetDevice(c->device));
  launch_shard_start(d_code, d_totals, rank, d_start_bit, c->stream);
  GHF_HIP(c, hipGetLastError());
  return GHF_OK;
}

int ghf_compress(ghf_ctx* c, const uint8_t* d_in, size_t n, uint8_t* d_out, size_t cap, uint64_t* d_out_bytes,
                 ghf_code* d_code, const ghf_index* index) {
  return ghf_compress_ex(c, d_in, n, d_out, cap, d_out_bytes, d_code, index, 0);
}

int ghf_compress_ex(ghf_ctx* c, const uint8_t* d_in, size_t n, uint8_t* d_out, size_t cap, uint64_t* d_out_bytes,
                    ghf_code* d_code, const ghf_index* index, unsigned code_flags) {
  if (!c || !d_out || (n && !d_in)) return GHF_E_INVAL;
  if (n == 0 && !(code_flags & GHF_EMPTY_OK)) return fail(c, GHF_E_EMPTY, "empty input is undefined in the reference; refused");
  if (!aligned16(d_out)) return fail(c, GHF_E_INVAL, "d_out must be 16-byte aligned");
  ghf_code* code = d_code ? d_code : c->d_code;
  int rc;
  if (n == 0) {
    // GHF_EMPTY_OK (include/ghf.h): header of the one-symbol code + the byte 0x7F.  No K4/K5: there is nothing to pack.
    const size_t hdr = ghf_header_bytes(1);
    if (cap < hdr + 1) return fail(c, GHF_E_CAP, "ghf_compress: capacity below the 1049 bytes of the empty stream");
    if ((rc = ghf_histogram(c, d_in, 0, c->d_hist))) return rc;
    if ((rc = ghf_build_code_ex(c, c->d_hist, code, code_flags))) return rc;
    if ((rc = ghf_write_header(c, code, d_out, cap))) return rc;
    GHF_HIP(c, hipMemsetAsync(d_out + hdr, 0x7F, 1, c->stream));
    if (d_out_bytes) {
      launch_store_u64(d_out_bytes, nullptr, hdr + 1, c->stream);
      GHF_HIP(c, hipGetLastError());
    }
    return GHF_OK;
  }
  if ((rc = ghf_histogram(c, d_in, n, c->d_hist))) return rc;   // compressor.h:63
  if ((rc = ghf_build_code_ex(c, c->d_hist, code, code_flags))) return rc;  // compressor.h:64
  if ((rc = ghf_encode_plan(c, d_in, n, code, &c->d->total_bits))) return rc;
  // compressor.h:70 + :72 -- the header rides along with the emit launches
  if ((rc = ghf_encode_emit(c, d_in, n, code, nullptr, GHF_EMIT_LAST | GHF_EMIT_HEADER, d_out, cap, index, c->d->end))) return rc;
  if (d_out_bytes) {
    launch_store_u64(d_out_bytes, &c->d->end[1], 0, c->stream);
    GHF_HIP(c, hipGetLastError());
  }
  return GHF_OK;
}

// ---------------------------------------------------------------------------------------------- index
int ghf_index_alloc(ghf_ctx* c, size_t n_symbols, ghf_index* out) {
  if (!c || !out) return GHF_E_INVAL;
  GHF_HIP(c, hipSetDevice(c->device));
  std::memset(out, 0, sizeof *out);
  index_shape(n_symbols, out);
  GHF_HIP(c, hipMalloc(&out->d_chunk_bit, std::max<size_t>(out->n_chunks, 1) * sizeof(uint64_t)));
  hipError_t e = hipMalloc(&out->d_seg_bit, std::max<size_t>(out->n_segs, 1) * sizeof(uint32_t));
  if (e != hipSuccess) {
    (void)hipFree(out->d_chunk_bit);
    out->d_chunk_bit = nullptr;
    return fail(c, GHF_E_HIP, "hipMalloc(seg_bit)", e);
  }
  return GHF_OK;
}

int ghf_index_free(ghf_ctx* c, ghf_index* idx) { return free_index_arrays(c, idx); }

// ---------------------------------------------------------------------------------------------- decode
static inline uint32_t be32(const uint8_t* p) {
  return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
}

// canonical_huff_encoder.cc:349-374, plus the validation the reference does not do: the rules of ghf_code_rules.h
// (section 1), which k_decode_images_batch applies to the same words on the device.
int ghf_parse_header(const uint8_t* h, size_t n, ghf_code* code, size_t* header_bytes) {
  if (!h || !code) return GHF_E_INVAL;
  if (n < kHeaderFixedBytes || !hdr_count_ok(be32(h))) return GHF_E_FORMAT;  // *code is untouched
  std::memset(code, 0, sizeof *code);
  for (int i = 0; i < GHF_NSYM; ++i) code->symbol[i] = be32(h + 4 * (1 + i));
  const uint8_t* p = h + 4 * (1 + GHF_NSYM);
  const uint32_t min_len = be32(p), max_len = be32(p + 4);
  if (!hdr_shape_ok(be32(h), min_len, max_len, n)) return GHF_E_FORMAT;
  code->min_len = (int32_t)min_len;
  code->max_len = (int32_t)max_len;
  p += 8;
  for (uint32_t i = 1; i <= max_len; ++i, p += 8) {
    code->start_pos[i] = be32(p);
    code->first_code[i] = be32(p + 4);
  }
  uint32_t used = 0;
  while (used < GHF_NSYM && code->symbol[used] != kSymUnused) ++used;
  bool seen[GHF_NSYM] = {false};  // the used symbols are all distinct, the end mark among them
  for (uint32_t i = 0; i < GHF_NSYM; ++i) {
    const uint32_t s = code->symbol[i];
    if (!hdr_symbol_ok(i, s, used) || (i < used && seen[s])) return GHF_E_FORMAT;
    if (i < used) seen[s] = true;
  }
  if (!seen[GHF_NSYM - 1]) return GHF_E_FORMAT;
  if (used == 1) {
    if (!hdr_lone_end_mark_ok((int)max_len, code->start_pos, code->first_code)) return GHF_E_FORMAT;
    code->length[GHF_NSYM - 1] = 1;
    code->codeword[GHF_NSYM - 1] = 0;
    if (header_bytes) *header_bytes = header_bytes_for(1);
    return GHF_OK;
  }
  // rebuild per-symbol lengths/codewords; the code must be the canonical complete prefix code
  unsigned long long kraft = 0;  // in units of 2^-32
  for (uint32_t len = 1; len <= max_len; ++len) {
    unsigned long long term;
    if (!hdr_len_ok((int)len, (int)min_len, (int)max_len, used, code->start_pos, code->first_code, &term)) return GHF_E_FORMAT;
    kraft += term;
    if (len < min_len) continue;
    const uint32_t a = code->start_pos[len], b = (len < max_len) ? code->start_pos[len + 1] : used;
    for (uint32_t r = 0; r < b - a; ++r) {
      const uint32_t s = code->symbol[a + r];
      code->length[s] = len;
      code->codeword[s] = code->first_code[len] + r;
    }
  }
  if (kraft != (1ull << 32)) return GHF_E_FORMAT;
  if (header_bytes) *header_bytes = header_bytes_for(max_len);
  return GHF_OK;
}

// ---- K6: rebuild the side-car of a stream that came without one (e.g. a .crs2 written by the reference) ----------
// Synchronises with the host a few times (convergence flag, symbol count); fills c->fidx.
struct RebuildRequest {
  const uint8_t* d_stream;
  size_t stream_bytes;
  SyncKind kind;
  uint64_t end_bit;           // one past the last bit that may belong to a code
  uint32_t first_start = 0;   // kSyncPiece: the first code boundary is assumed this many bits behind hdr
  size_t hdr = 0;             // bytes in front of the first code
  int max_len = 0;            // the longest code, for the stride of the scan's function rows
  bool scan_at_once = false;  // a near-fixed-length code: seed the boundaries with the deterministic scan before any pass
  size_t cap = (size_t)-1;    // decoded bytes the caller has room for
};

struct RebuildResult {
  uint64_t n = 0;             // symbols: codes that start in front of end_bit, up to the end mark
  uint64_t landing = 0;       // kSyncPiece: bits the last code runs past end_bit
  bool has_end_mark = false;  // kSyncPiece: the piece holds one
};

// cuts c->sync into K6's arrays for p.nsub subsequences; *scan_ws: the deterministic scan's share
static int carve_sync_workspace(ghf_ctx* c, SyncParams& p, uint8_t** scan_ws) {
  const size_t ntiles = (p.nsub + 255) / 256;
  size_t off = 0;
  auto carve = [&](size_t bytes) {
    const size_t o = off;
    off += (bytes + 255) & ~(size_t)255;
    return o;
  };
  const size_t o_start = carve((p.nsub + 1) * 2), o_used = carve(p.nsub * 2), o_cnt = carve(p.nsub * 4), o_eof = carve(p.nsub),
               o_tile = carve((ntiles + 2) * 8), o_scan = carve(sync_scan_workspace(p.nsub));
  const int rc = grow(c, c->sync, off);
  if (rc) return rc;
  uint8_t* ws = c->sync.p;
  p.start = reinterpret_cast<uint16_t*>(ws + o_start);
  p.used = reinterpret_cast<uint16_t*>(ws + o_used);
  p.cnt = reinterpret_cast<uint32_t*>(ws + o_cnt);
  p.eof = ws + o_eof;
  p.tile_sum = reinterpret_cast<uint64_t*>(ws + o_tile);
  *scan_ws = ws + o_scan;
  return GHF_OK;
}

// seeds the boundary guesses and queues passes until none moves; the last batch's read-back is left in c->h->k6
static int settle_boundaries(ghf_ctx* c, SyncParams& p, uint8_t* scan_ws, const RebuildRequest& q) {
  // the stride of the scan's function rows (launch_sync_scan): a shallow code does not pay for 64-byte rows
  const uint32_t stride = (q.max_len >= 1 && q.max_len <= 16) ? 16u : (q.max_len > 32 ? 64u : 32u);
  bool scanned = q.first_start >= stride;  // (the scan follows entry offsets below its stride only: such a piece counts as seeded)
  // (An entry offset in [max_len, stride) -- no true boundary lies there, only a caller's wrong guess -- indexes a row entry
  //  that k_sync_table does not write: class rows hold counts there, other rows whatever the workspace held.  The scan then
  //  seeds start[] with values that depend on stale memory; the passes repair them, one subsequence per pass, within the bound
  //  below, so the result is right and only the number of passes varies.)
  const bool scan_first = q.scan_at_once && !scanned;
  p.first = scan_first ? 0u : 3u;
  p.first_start = q.first_start;
  // `start`, `used`, `eof` (11 bytes per KiB of stream: 3 + 3 + 1.5 MB at 256 MiB) are not cleared when the fixed-point passes
  // come first: the first k_sync_pass of the call finds every subsequence unworked and every guess 0 because its parameters
  // say so (SyncParams::first), and writes all three arrays whole.  (Round 3 queued three memsets, 60 us at 256 MiB in front
  // of a 1 ms job.)
  if (scan_first) {
    // (the scan's kernels write the guesses they derive -- and, for the subsequences whose class walk already is the whole
    //  answer, the results too: `used` must say "nothing yet" for all the others)
    GHF_HIP(c, hipMemsetAsync(p.start, 0, (p.nsub + 1) * 2, c->stream));
    if (q.first_start) launch_store_u64(reinterpret_cast<uint64_t*>(p.start), nullptr, q.first_start, c->stream);  // start[0]
    GHF_HIP(c, hipMemsetAsync(p.used, 0xFF, p.nsub * 2, c->stream));
    GHF_HIP(c, hipMemsetAsync(p.eof, 0, p.nsub, c->stream));
    launch_sync_scan(p, scan_ws, stride, q.first_start, c->stream);  // (seeds the boundaries; the passes below only verify)
    scanned = true;
  } else {
    launch_store_u64(reinterpret_cast<uint64_t*>(p.start), nullptr, q.first_start, c->stream);  // start[0] (k_sync_pass stores start[1 ..])
  }
  // passes until no boundary guess moves (self-synchronisation: a handful of passes in practice).  They are queued in
  // batches; behind every batch the counts (first end mark, symbols per tile, their scan) and the landing bit are queued as
  // well, and the host reads {symbols, end-mark subsequence, "something moved", landing} in ONE round trip: a stream that has
  // settled in its first batch -- the usual case, and the rule behind the deterministic scan -- costs one synchronisation (round 2:
  // four per call, a quarter of the file decompressor's K6 time at 16 MiB pieces).
  // Streams that self-synchronise slowly (near-fixed-length codes) would need one pass per subsequence of drift: their
  // boundaries are seeded by the deterministic scan (launch_sync_scan) -- at once when the caller knows the code is of that
  // kind, otherwise as soon as a first batch of passes has not settled.  The passes then only verify.
  constexpr int kBatch = 4;
  const K6Readback& k = c->h->k6;
  for (uint64_t passes = 0;;) {
    if (passes > p.nsub + 2) return fail(c, GHF_E_CORRUPT, "self-synchronisation did not converge");
    // (behind the deterministic scan the first pass only has to CONFIRM the boundaries: one pass, not a batch)
    const int nb = (scanned && passes == 0) ? 1 : kBatch;
    for (int b = 0; b < nb; ++b) {
      GHF_HIP(c, hipMemsetAsync(&c->d->k6.moved, 0, sizeof(K6Moved), c->stream));  // flag, count, first (inverted)
      launch_sync_pass(p, c->stream);
      p.first = 0;
    }
    passes += nb;
    launch_store_u64(p.eof_sub, nullptr, p.nsub, c->stream);  // "none found"; k_sync_eof takes the minimum
    launch_sync_counts(p, &c->d->k6.n_symbols, c->stream);
    launch_load_u16(&c->d->k6.landing, p.start + p.nsub, c->stream);
    GHF_HIP(c, hipMemcpyAsync(&c->h->k6, &c->d->k6, sizeof(K6Readback), hipMemcpyDeviceToHost, c->stream));
    GHF_HIP(c, hipStreamSynchronize(c->stream));
    const uint64_t moved = (uint64_t)k.moved.changed[1] * 256;  // boundaries the batch's last pass moved (sampled: every 256th group)
#ifdef GHF_K6_TRACE  // (scratch/build_variant.sh k6trace -DGHF_K6_TRACE: what every batch of passes left behind)
    fprintf(stderr, "[k6] nsub %llu passes %llu scanned %d flag %u moved~%llu first %llu eof_sub %llu\n", (unsigned long long)p.nsub,
            (unsigned long long)passes, (int)scanned, (unsigned)k.moved.changed[0], (unsigned long long)moved,
            (unsigned long long)~k.moved.first_inv, (unsigned long long)k.eof_sub);
#endif
    if (k.moved.changed[0] == 0) break;
    // .crs2: settled IN FRONT OF THE END MARK is settled.  No landing at or before the first end mark's subsequence moved
    // in the batch's last pass -> every boundary up to it is a fixed point, the mark is the stream's (the first one, and
    // real).  What lies behind it (a buffer longer than its stream: stale bytes) may go on moving for ever.
    if (q.kind == kSyncCrs2 && k.moved.first_inv != 0 && ~k.moved.first_inv >= k.eof_sub && k.eof_sub < p.nsub) break;
    // Not settled.  A boundary that is still moving travels ONE subsequence to the right per pass, and a pass in which
    // little moved costs little (a wave whose 64 subsequences are current skips them), so a few more batches are cheaper
    // than the deterministic scan over the whole stream -- which long streams of a quickly synchronising code otherwise
    // fall into because SOME stretch among their millions of subsequences needs a fifth pass (4 GiB Zipf: 44 ms with
    // the scan after the first batch, see profiles/r04/foreign_4GiB.txt).  Codes that do not settle in kScanAfter passes
    // (long runs of one value, near-fixed-length codes the caller did not announce) get the scan then.
    // What decides is HOW MUCH still moves: a few stragglers (one stretch in a 4 GiB Zipf stream needs 17..20 passes,
    // whichever seed) are followed for up to kScanAfterFew passes; a stream in which boundaries still move everywhere
    // after two batches is not going to settle by itself.
    constexpr uint64_t kScanAfterMany = 8, kScanAfterFew = 64;
    const uint64_t few = p.nsub >> 10 > 4096 ? p.nsub >> 10 : 4096;
    if (!scanned && (passes >= kScanAfterFew || (passes >= kScanAfterMany && moved > few))) {
      launch_sync_scan(p, scan_ws, stride, q.first_start, c->stream);
      scanned = true;
    }
  }
  return GHF_OK;
}

// sizes c->fidx for n symbols and queues the kernel that fills it from the settled boundaries
static int build_sidecar(ghf_ctx* c, const SyncParams& p, uint64_t n, uint32_t flags) {
  const uint64_t n_chunks = blocks_for(n), n_segs = segs_for(n);
  ghf_index& ix = c->fidx;
  if (n) {  // (d_seg_abs has one entry more than there are segments)
    int rc = grow(c, c->seg_bit, n_segs);
    if (!rc) rc = grow(c, c->seg_abs, n_segs + 1);
    if (!rc) rc = grow(c, c->chunk_bit, n_chunks);
    ix.d_seg_bit = c->seg_bit.p;
    ix.d_chunk_bit = c->chunk_bit.p;
    if (rc) return rc;
  }
  index_shape(n, &ix);
  ix.flags = flags;
  if (n) launch_sync_index(p, c->seg_abs.p, n, ix.d_chunk_bit, ix.d_seg_bit, c->stream);
  GHF_HIP(c, hipGetLastError());
  return GHF_OK;
}

static int rebuild_index_at(ghf_ctx* c, const RebuildRequest& q, RebuildResult* r /* may be null */) {
  SyncParams p;
  p.stream = q.d_stream;
  p.stream_bytes = q.stream_bytes;
  p.body_bit0 = (uint64_t)q.hdr * 8;
  p.end_bit = q.end_bit;
  p.no_eof = q.kind;
  p.dt = c->d_dt;
  p.nsub = (q.end_bit - p.body_bit0 + 511) / 512;
  p.changed = c->d->k6.moved.changed;
  p.moved_first_inv = &c->d->k6.moved.first_inv;
  p.eof_sub = &c->d->k6.eof_sub;
  uint8_t* scan_ws = nullptr;
  int rc = carve_sync_workspace(c, p, &scan_ws);
  if (!rc) rc = settle_boundaries(c, p, scan_ws, q);
  if (rc) return rc;
  const uint64_t n = c->h->k6.n_symbols;
  const uint16_t land16 = (uint16_t)c->h->k6.landing;  // 0xFFFF: the last subsequence ended at an end mark (real, or a fake one of a wrong guess)
  const bool has_end_mark = c->h->k6.eof_sub < p.nsub;
  // .crs: every subsequence counts; a flagged one means bits that are no code or a code running past the end
  // (eof_sub == nsub, "none", makes the counting kernels take every subsequence: n is already the total)
  if (q.kind == kSyncCrs && has_end_mark) return fail(c, GHF_E_CORRUPT, "the .crs body does not end on a code boundary");
  if (q.kind == kSyncCrs2 && !has_end_mark) return fail(c, GHF_E_CORRUPT, "no end mark in the stream");
  if (n > q.cap) return fail(c, GHF_E_CAP, "ghf_decode: output capacity below the decoded size");
  rc = build_sidecar(c, p, n, (q.kind == kSyncPiece && !has_end_mark) ? (uint32_t)GHF_INDEX_NO_END_MARK : 0u);
  if (rc) return rc;
  c->rebuilt = {q.d_stream, q.stream_bytes};
  if (r) *r = {n, land16 == 0xFFFF ? 0u : land16, has_end_mark};
  return GHF_OK;
}

// a whole .crs2: the header's length and the kind of code come from the device-resident tables
static int rebuild_index(ghf_ctx* c, const uint8_t* d_stream, size_t stream_bytes, const ghf_code* d_code, size_t cap) {
  ghf_code* hc = new (std::nothrow) ghf_code;
  if (!hc) return GHF_E_NOMEM;
  hipError_t e = hipMemcpyAsync(hc, d_code, sizeof(ghf_code), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  const int max_len = hc->max_len, min_len = hc->min_len;
  delete hc;
  if (e != hipSuccess) return fail(c, GHF_E_HIP, "copy tables to host", e);
  if (max_len < 1 || max_len > 32) return fail(c, GHF_E_FORMAT, "bad max_len in tables");
  RebuildRequest q{d_stream, stream_bytes, kSyncCrs2, (uint64_t)stream_bytes * 8};
  q.hdr = ghf_header_bytes(max_len);
  if (stream_bytes <= q.hdr) return fail(c, GHF_E_FORMAT, "stream shorter than its header");
  q.max_len = max_len;
  q.scan_at_once = max_len - min_len <= 1;
  q.cap = cap;
  return rebuild_index_at(c, q, nullptr);
}

// the depth of a device-resident tree (1..64), for the stride of K6's function rows: 16 / 32 / 64 bytes as for .crs2 -- a
// shallow tree does not pay for 64-byte rows -- and, where the caller asks for it, tree_bytes; one round trip
static int crs_tree_shape(ghf_ctx* c, const ghf_tree* d_tree, uint32_t* tree_bytes, int* max_len) {
  hipError_t e = hipSuccess;
  if (tree_bytes) e = hipMemcpyAsync(&c->h->tree_bytes, &d_tree->tree_bytes, sizeof(d_tree->tree_bytes), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(&c->h->tree_max_len, &d_tree->max_len, sizeof(d_tree->max_len), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(c, GHF_E_HIP, tree_bytes ? "copy tree_bytes to host" : "copy the tree's max_len to host", e);
  if (tree_bytes) *tree_bytes = c->h->tree_bytes;
  const uint32_t ml = c->h->tree_max_len;
  *max_len = (ml >= 1 && ml <= 64) ? (int)ml : 64;  // (anything else is refused by k_crs_decode_tables)
  return GHF_OK;
}

// Multi-GPU decode of a side-car-less stream and the file pipeline's .crs pieces: one piece.  Rebuilds the
// piece's side-car and keeps it for the following decode with index = NULL of the same (d_piece, bytes).
// ghf_sync_piece (canonical tables at d_code) and ghf_crs_sync_piece (d_tree): one of the two is given.
// q: the piece, its first_start and end_bit as the caller gave them; the code's shape is filled in here.
static int sync_piece(ghf_ctx* c, const char* who, RebuildRequest q, const ghf_code* d_code, const ghf_tree* d_tree, RebuildResult* r) {
  if (!aligned16(q.d_stream)) return fail(c, GHF_E_INVAL, "d_piece must be 16-byte aligned");
  if (q.first_start >= 512 || q.end_bit > (uint64_t)q.stream_bytes * 8 || q.first_start > q.end_bit)
    return fail(c, GHF_E_INVAL, (std::string(who) + ": bad first_bit / end_bit").c_str());
  GHF_HIP(c, hipSetDevice(c->device));
  if (d_code) launch_build_decode_tables(d_code, c->d_dt, c->d_status, c->stream);
  else launch_crs_decode_tables(d_tree, c->d_dt, c->d_status, c->stream);
  c->prepared.forget();
  c->rebuilt.forget();
  if (q.end_bit == 0) {  // nothing of this piece is its own
    c->fidx.n_symbols = 0;
    c->fidx.n_segs = 0;
    c->fidx.n_chunks = 0;
    c->rebuilt = {q.d_stream, q.stream_bytes};
    return GHF_OK;
  }
  if (d_code) {
    // near-fixed-length codes re-synchronise slowly: the deterministic scan seeds the boundaries at once (as in rebuild_index)
    GHF_HIP(c, hipMemcpyAsync(c->h->code_lens, &d_code->min_len, sizeof c->h->code_lens, hipMemcpyDeviceToHost, c->stream));
    GHF_HIP(c, hipStreamSynchronize(c->stream));
    const int32_t min_len = c->h->code_lens[0], max_len = c->h->code_lens[1];
    if (!len_bounds_ok(min_len, max_len)) return fail(c, GHF_E_FORMAT, "bad min_len / max_len in tables");
    q.max_len = max_len;
    q.scan_at_once = max_len - min_len <= 1;
  } else {
    const int rc = crs_tree_shape(c, d_tree, nullptr, &q.max_len);
    if (rc) return rc;
  }
  return rebuild_index_at(c, q, r);
}

int ghf_sync_piece(ghf_ctx* c, const uint8_t* d_piece, size_t piece_bytes, uint32_t first_bit, uint64_t end_bit,
                   const ghf_code* d_code, uint64_t* landing, uint64_t* n_symbols, int* has_end_mark) {
  if (!c || !d_piece || !d_code || !landing || !n_symbols || !has_end_mark) return GHF_E_INVAL;
  RebuildResult r;
  const int rc = sync_piece(c, "ghf_sync_piece", RebuildRequest{d_piece, piece_bytes, kSyncPiece, end_bit, first_bit}, d_code, nullptr, &r);
  *landing = r.landing;
  *n_symbols = r.n;
  *has_end_mark = r.has_end_mark;
  return rc;
}

int ghf_decoded_size(ghf_ctx* c, const uint8_t* d_stream, size_t stream_bytes, const ghf_code* d_code, uint64_t* n_out) {
  if (!c || !d_stream || !d_code || !n_out) return GHF_E_INVAL;
  if (!aligned16(d_stream)) return fail(c, GHF_E_INVAL, "d_stream must be 16-byte aligned");
  GHF_HIP(c, hipSetDevice(c->device));
  launch_build_decode_tables(d_code, c->d_dt, c->d_status, c->stream);
  c->prepared.forget();
  c->rebuilt.forget();
  const int rc = rebuild_index(c, d_stream, stream_bytes, d_code, (size_t)-1);
  if (rc) return rc;
  *n_out = c->fidx.n_symbols;
  return GHF_OK;
}

int ghf_decode_prepare(ghf_ctx* c, const ghf_code* d_code) {
  if (!c || !d_code) return GHF_E_INVAL;
  GHF_HIP(c, hipSetDevice(c->device));
  launch_build_decode_tables(d_code, c->d_dt, c->d_status, c->stream);
  GHF_HIP(c, hipGetLastError());
  c->prepared = {d_code};
  return GHF_OK;
}

// nothing to decode (the end mark comes first: GHF_EMPTY_OK's stream, a shard or a piece that holds nothing; an empty .crs body): no K7
static int nothing_decoded(ghf_ctx* c, uint64_t* d_out_bytes) {
  if (d_out_bytes) launch_store_u64(d_out_bytes, nullptr, 0, c->stream);
  GHF_HIP(c, hipGetLastError());
  return GHF_OK;
}

// What ghf_decode and ghf_crs_decode (`who`) share once d_dt is queued and the side-car is chosen: K7.
// p: stream, stream_bytes, out, out_bytes and no_end_mark as the caller has them; the rest is filled here.
static int decode_with_index(ghf_ctx* c, const char* who, const ghf_index* index, size_t cap, DecParams p) {
  const std::string f = std::string(who) + ": ";
  if (!index_matches_n(index)) return fail(c, GHF_E_INVAL, (f + "malformed index").c_str());
  if (cap < index->n_symbols) return fail(c, GHF_E_CAP, (f + "output capacity below n_symbols").c_str());
  if (index->n_chunks >= kDecMaxGroups) return fail(c, GHF_E_INVAL, (f + "more than 2^44 symbols in one call").c_str());
  p.dt = c->d_dt;
  p.chunk_bit = index->d_chunk_bit;
  p.seg_bit = index->d_seg_bit;
  p.n_symbols = index->n_symbols;
  p.n_segs = index->n_segs;
  p.status = c->d_status;
  launch_decode(p, c->stream);
  if (p.out_bytes && index->n_symbols == 0) launch_store_u64(p.out_bytes, nullptr, 0, c->stream);  // no decode launch then
  GHF_HIP(c, hipGetLastError());
  return GHF_OK;
}

int ghf_decode(ghf_ctx* c, const uint8_t* d_stream, size_t stream_bytes, const ghf_code* d_code,
               const ghf_index* index, uint8_t* d_out, size_t cap, uint64_t* d_out_bytes) {
  if (!c || !d_stream || !d_code || !d_out) return GHF_E_INVAL;
  if (!aligned16(d_stream)) return fail(c, GHF_E_INVAL, "d_stream must be 16-byte aligned");
  GHF_HIP(c, hipSetDevice(c->device));
  // prepared: single use (the tables also hold this decode's work counters)
  if (!(c->prepared.describes(d_code) && index)) launch_build_decode_tables(d_code, c->d_dt, c->d_status, c->stream);
  c->prepared.forget();
  if (!index) {
    if (!c->rebuilt.describes(d_stream, stream_bytes)) {  // else: ghf_decoded_size / ghf_sync_piece already did it
      const int rc = rebuild_index(c, d_stream, stream_bytes, d_code, cap);
      if (rc) return rc;
    }
    c->rebuilt.forget();  // single use: the buffer may be rewritten afterwards
    index = &c->fidx;
  }
  if (index->n_symbols == 0) return nothing_decoded(c, d_out_bytes);
  DecParams p = {};
  p.stream = d_stream;
  p.stream_bytes = stream_bytes;
  p.no_end_mark = (index->flags & GHF_INDEX_NO_END_MARK) ? 1u : 0u;
  p.out = d_out;
  p.out_bytes = d_out_bytes;
  return decode_with_index(c, "ghf_decode", index, cap, p);
}

// ---------------------------------------------------------------------------------------------- seek table
// (no reference counterpart; the format: DESIGN.md "Seekable .crs2")
size_t ghf_seek_bytes(size_t n_symbols) { return kSeekHeaderBytes + kSeekRecordBytes * (size_t)blocks_for(n_symbols); }

int ghf_seek_parse(const uint8_t* h, size_t bytes, ghf_seek_info* info) {
  if (!h || !info) return GHF_E_INVAL;
  std::memset(info, 0, sizeof *info);
  if (bytes < kSeekHeaderBytes) return GHF_E_FORMAT;
  if (le64(h) != kSeekMagic || le32(h + 8) != kSeekVersion) return GHF_E_FORMAT;
  const uint32_t flags = le32(h + 12);
  const uint64_t n = le64(h + 16), n_blocks = le64(h + 32);
  if (flags & ~(uint32_t)GHF_INDEX_NO_END_MARK) return GHF_E_FORMAT;
  if (le32(h + 24) != (uint32_t)kBlockSymbols || le32(h + 28) != (uint32_t)kRunSymbols) return GHF_E_FORMAT;
  if (n_blocks != blocks_for(n) || n_blocks >= kDecMaxGroups) return GHF_E_FORMAT;
  for (size_t i = 40; i < kSeekHeaderBytes; ++i)
    if (h[i]) return GHF_E_FORMAT;
  if (bytes != kSeekHeaderBytes + kSeekRecordBytes * (size_t)n_blocks) return GHF_E_FORMAT;  // truncated, or something behind it
  info->n_symbols = n;
  info->n_blocks = n_blocks;
  info->flags = flags;
  info->version = kSeekVersion;
  return GHF_OK;
}

int ghf_seek_pack(ghf_ctx* c, const ghf_index* index, const uint8_t* d_stream, size_t stream_bytes, uint8_t* d_table, size_t cap) {
  if (!c || !d_table) return GHF_E_INVAL;
  if (!aligned16(d_table) || !aligned16(d_stream)) return fail(c, GHF_E_INVAL, "ghf_seek_pack: d_stream and d_table must be 16-byte aligned");
  if (!index) {  // the side-car K6 last rebuilt on this context, while it still describes this buffer
    if (!d_stream || !c->rebuilt.describes(d_stream, stream_bytes))
      return fail(c, GHF_E_INVAL, "ghf_seek_pack: no rebuilt side-car for this stream (call ghf_decoded_size first)");
    index = &c->fidx;
  }
  if (index->n_symbols != 0 && !index_is_whole(index)) return fail(c, GHF_E_INVAL, "ghf_seek_pack: malformed index");
  if (cap < ghf_seek_bytes(index->n_symbols)) return fail(c, GHF_E_CAP, "ghf_seek_pack: table capacity below ghf_seek_bytes(n_symbols)");
  GHF_HIP(c, hipSetDevice(c->device));
  SeekPackParams p = {};
  p.chunk_bit = index->d_chunk_bit;
  p.seg_bit = index->d_seg_bit;
  p.n_symbols = index->n_symbols;
  p.n_blocks = blocks_for(index->n_symbols);
  p.n_segs = segs_for(index->n_symbols);
  p.flags = index->flags & (uint32_t)GHF_INDEX_NO_END_MARK;
  p.table = d_table;
  p.status = c->d_status;
  launch_seek_pack(p, c->stream);
  GHF_HIP(c, hipGetLastError());
  return GHF_OK;
}

// queues k_seek_expand for blocks [g0, g1) of the table; d_dt must already be queued
static void expand_blocks(ghf_ctx* c, const ghf_seek_info* info, const uint8_t* d_table, const uint8_t* d_stream, size_t stream_bytes,
                          uint64_t g0, uint64_t g1, uint64_t* d_chunk_bit, uint32_t* d_seg_bit) {
  launch_seek_expand(seek_expand_params(c, info, d_table, d_stream, stream_bytes, c->d_dt, g0, g1, d_chunk_bit, d_seg_bit), c->stream);
}

int ghf_seek_expand(ghf_ctx* c, const ghf_seek_info* info, const uint8_t* d_table, size_t table_bytes, const uint8_t* d_stream,
                    size_t stream_bytes, const ghf_code* d_code, ghf_index* index) {
  if (!c || !info || !d_table || !d_stream || !d_code || !index) return GHF_E_INVAL;
  if (!aligned16(d_stream)) return fail(c, GHF_E_INVAL, "ghf_seek_expand: d_stream must be 16-byte aligned");
  int rc = seek_table_ok(c, "ghf_seek_expand", info, d_table, table_bytes);
  if (rc) return rc;
  if (index->n_symbols != info->n_symbols || (info->n_symbols != 0 && !index_is_whole(index)))
    return fail(c, GHF_E_INVAL, "ghf_seek_expand: the index was not allocated for the table's n_symbols");
  GHF_HIP(c, hipSetDevice(c->device));
  index->flags = info->flags;
  if (info->n_blocks == 0) return GHF_OK;
  launch_build_decode_tables(d_code, c->d_dt, c->d_status, c->stream);
  c->prepared.forget();
  expand_blocks(c, info, d_table, d_stream, stream_bytes, 0, info->n_blocks, index->d_chunk_bit, index->d_seg_bit);
  GHF_HIP(c, hipGetLastError());
  return GHF_OK;
}

int ghf_decode_range(ghf_ctx* c, const uint8_t* d_stream, size_t stream_bytes, const ghf_code* d_code, const ghf_index* index,
                     const ghf_seek_info* info, const uint8_t* d_table, size_t table_bytes, uint64_t first, uint64_t count,
                     uint8_t* d_out, size_t cap) {
  if (!c || !d_stream || !d_code) return GHF_E_INVAL;
  if (!aligned16(d_stream)) return fail(c, GHF_E_INVAL, "ghf_decode_range: d_stream must be 16-byte aligned");
  const bool by_table = info || d_table;
  if ((index != nullptr) == by_table || (by_table && !(info && d_table)))
    return fail(c, GHF_E_INVAL, "ghf_decode_range: exactly one of index / (info, d_table) must be given");
  uint64_t n = 0;
  uint32_t flags = 0;
  if (by_table) {
    const int rc = seek_table_ok(c, "ghf_decode_range", info, d_table, table_bytes);
    if (rc) return rc;
    n = info->n_symbols;
    flags = info->flags;
  } else {
    if (index->n_symbols != 0 && !index_is_whole(index)) return fail(c, GHF_E_INVAL, "ghf_decode_range: malformed index");
    n = index->n_symbols;
    flags = index->flags;
  }
  if (first > n || count > n - first) return fail(c, GHF_E_INVAL, "ghf_decode_range: first + count exceeds n_symbols");
  if (cap < count) return fail(c, GHF_E_CAP, "ghf_decode_range: output capacity below count");
  if (count == 0) return GHF_OK;
  if (!d_out) return GHF_E_INVAL;
  GHF_HIP(c, hipSetDevice(c->device));
  const uint64_t end = first + count;
  const uint64_t gA = first / kBlockSymbols, gB = blocks_for(end);  // the covered blocks [gA, gB)
  launch_build_decode_tables(d_code, c->d_dt, c->d_status, c->stream);
  c->prepared.forget();
  const uint64_t* chunk_bit;
  const uint32_t* seg_bit;
  if (by_table) {  // only the covered blocks are expanded
    int rc = grow(c, c->range_chunk, gB - gA, 1024);
    if (!rc) rc = grow(c, c->range_seg, (gB - gA) * (kBlockSymbols / kSegSymbols), 1024 * 64);
    if (rc) return rc;
    expand_blocks(c, info, d_table, d_stream, stream_bytes, gA, gB, c->range_chunk.p, c->range_seg.p);
    chunk_bit = c->range_chunk.p;
    seg_bit = c->range_seg.p;
  } else {
    chunk_bit = index->d_chunk_bit + gA;
    seg_bit = index->d_seg_bit + gA * (kBlockSymbols / kSegSymbols);
  }
  uint64_t gI = gA;  // the first block K7 takes
  if (first % kBlockSymbols) {
    DecHeadParams h = {};
    h.stream = d_stream;
    h.stream_bytes = stream_bytes;
    h.dt = c->d_dt;
    h.chunk_bit = chunk_bit;
    h.seg_bit = seg_bit;
    h.blk_sym0 = gA * kBlockSymbols;
    h.n_symbols = n;
    h.lo = first;
    h.hi = std::min<uint64_t>(end, (gA + 1) * kBlockSymbols);
    h.out = d_out;
    h.status = c->d_status;
    launch_decode_head(h, c->stream);
    gI = gA + 1;
  }
  if (end > gI * kBlockSymbols)  // K7 on the view of the side-car that begins at block gI and ends with the range
    launch_decode(range_decode_params(c, d_stream, stream_bytes, c->d_dt, chunk_bit + (gI - gA),
                                      seg_bit + (gI - gA) * (kBlockSymbols / kSegSymbols), gI, end, n, flags,
                                      d_out + (gI * kBlockSymbols - first)),
                  c->stream);
  GHF_HIP(c, hipGetLastError());
  return GHF_OK;
}

// ---------------------------------------------------------------------------------------------- .crs
int ghf_crs_build_code(ghf_ctx* c, const uint64_t* d_hist, ghf_tree* d_tree, ghf_code* d_code) {
  if (!c || !d_hist || !d_tree || !d_code) return GHF_E_INVAL;
  GHF_HIP(c, hipSetDevice(c->device));
  launch_crs_build_code(d_hist, d_tree, d_code, &c->d->start_bit, c->d_status, c->stream);
  GHF_HIP(c, hipGetLastError());
  c->plan.forget();  // d_code changed: a cached plan no longer describes it
  if (c->prepared.describes(d_code)) c->prepared.forget();  // ... and neither do decode tables prepared from it
  return GHF_OK;
}

size_t ghf_crs_compress_bound(size_t n) { return 1024 + 2 + ghf_compress_bound(n); }

int ghf_crs_compress(ghf_ctx* c, const uint8_t* d_in, size_t n, uint8_t* d_out, size_t cap, uint64_t* d_out_bytes,
                     ghf_tree* d_tree, const ghf_index* index) {
  if (!c || !d_out || (n && !d_in)) return GHF_E_INVAL;
  if (n == 0) return fail(c, GHF_E_EMPTY, "empty input is undefined in the reference; refused");
  if (!aligned16(d_out)) return fail(c, GHF_E_INVAL, "d_out must be 16-byte aligned");
  ghf_tree* tree = d_tree ? d_tree : c->d_tree;
  int rc;
  if ((rc = ghf_histogram(c, d_in, n, c->d_hist))) return rc;            // compressor.h:63
  if ((rc = ghf_crs_build_code(c, c->d_hist, tree, c->d_code))) return rc;  // compressor.h:64, start bit -> d->start_bit
  if ((rc = ghf_encode_plan(c, d_in, n, c->d_code, &c->d->total_bits))) return rc;
  // compressor.h:72: the body right behind tree + two prefix bytes; no end mark, zero fill (flags = 0)
  if ((rc = ghf_encode_emit(c, d_in, n, c->d_code, &c->d->start_bit, GHF_EMIT_LONG_CODES, d_out, cap, index, c->d->end))) return rc;
  launch_crs_finish(tree, &c->d->total_bits, d_out, d_out_bytes, c->d_status, c->stream);  // compressor.h:70 + normal_huff_encoder.h:176-184
  GHF_HIP(c, hipGetLastError());
  return GHF_OK;
}

// DecodeHuffTree::do_build_tree (include/huff_tree.cc:289-303), iteratively and with bounds
int ghf_crs_parse_header(const uint8_t* h, size_t n, ghf_tree* tree, size_t* tree_bytes) {
  if (!h || !tree) return GHF_E_INVAL;
  std::memset(tree, 0, sizeof *tree);
  struct Open {  // a parent that still waits for a child
    uint16_t idx, depth;
    bool has_left;
  };
  Open stack[260];
  int sp = 0;
  size_t pos = 0;
  uint32_t n_parents = 0, n_leaves = 0, max_len = 0;
  for (bool first_node = true;; first_node = false) {
    if (pos + 2 > n || pos + 2 > sizeof tree->header) return GHF_E_FORMAT;
    const bool leaf = h[pos] == 0;  // huff_tree.cc:294: first byte 0 = leaf, second byte = key
    const uint32_t key = h[pos + 1];
    pos += 2;
    uint32_t id, depth = 0;
    if (leaf) {
      id = key;
      ++n_leaves;
    } else {
      if (n_parents >= 255) return GHF_E_FORMAT;
      id = 256 + n_parents++;
    }
    if (first_node) {
      if (leaf) return GHF_E_FORMAT;  // the root is a leaf: the reference's decoder dereferences NULL there
      tree->root = id;
    } else {
      Open& top = stack[sp - 1];
      depth = top.depth + 1u;
      if (!top.has_left) {
        tree->left[top.idx] = (uint16_t)id;
        top.has_left = true;
      } else {
        tree->right[top.idx] = (uint16_t)id;
        --sp;
      }
    }
    if (leaf) {
      if (depth > max_len) max_len = depth;
    } else {
      if (sp >= 258) return GHF_E_FORMAT;
      stack[sp].idx = (uint16_t)(id - 256);
      stack[sp].depth = (uint16_t)depth;
      stack[sp].has_left = false;
      ++sp;
    }
    if (sp == 0) break;
  }
  if (n_leaves < 2 || n_leaves > 256 || n_parents != n_leaves - 1) return GHF_E_FORMAT;
  if (max_len > 64) return GHF_E_CODELEN;  // (a tree that deep needs more than 2^44 input bytes)
  tree->n_leaves = n_leaves;
  tree->max_len = max_len;
  tree->tree_bytes = (uint32_t)pos;
  std::memcpy(tree->header, h, pos);
  if (tree_bytes) *tree_bytes = pos;
  return GHF_OK;
}

// where the body of a whole .crs lies and how deep its tree is: the request for its side-car (cap is the caller's)
static int crs_request(ghf_ctx* c, const uint8_t* d_stream, size_t stream_bytes, int left_bits, const ghf_tree* d_tree, RebuildRequest* q) {
  if (left_bits < 0 || left_bits > 7) return fail(c, GHF_E_FORMAT, "left_bits must be 0..7");
  uint32_t tb = 0;
  *q = RebuildRequest{d_stream, stream_bytes, kSyncCrs, (uint64_t)stream_bytes * 8 - (uint64_t)left_bits};
  const int rc = crs_tree_shape(c, d_tree, &tb, &q->max_len);  // (codes up to 64 bits)
  if (rc) return rc;
  if (tb < 6 || tb > 1022 || (tb & 1)) return fail(c, GHF_E_FORMAT, "bad tree_bytes");
  q->hdr = (size_t)tb + 2;
  if (stream_bytes < q->hdr || (left_bits && stream_bytes == q->hdr)) return fail(c, GHF_E_FORMAT, "stream shorter than its header");
  return GHF_OK;
}

int ghf_crs_decoded_size(ghf_ctx* c, const uint8_t* d_stream, size_t stream_bytes, int left_bits, const ghf_tree* d_tree,
                         uint64_t* n_out) {
  if (!c || !d_stream || !d_tree || !n_out) return GHF_E_INVAL;
  if (!aligned16(d_stream)) return fail(c, GHF_E_INVAL, "d_stream must be 16-byte aligned");
  GHF_HIP(c, hipSetDevice(c->device));
  RebuildRequest q;
  int rc = crs_request(c, d_stream, stream_bytes, left_bits, d_tree, &q);
  if (rc) return rc;
  launch_crs_decode_tables(d_tree, c->d_dt, c->d_status, c->stream);
  c->prepared.forget();
  RebuildResult r;  // an empty body decodes to nothing
  if (q.end_bit != (uint64_t)q.hdr * 8) {
    rc = rebuild_index_at(c, q, &r);
    if (rc) return rc;
  }
  *n_out = r.n;
  return GHF_OK;
}

int ghf_crs_sync_piece(ghf_ctx* c, const uint8_t* d_piece, size_t piece_bytes, uint32_t first_bit, uint64_t end_bit,
                       const ghf_tree* d_tree, uint64_t* landing, uint64_t* n_symbols) {
  if (!c || !d_piece || !d_tree || !landing || !n_symbols) return GHF_E_INVAL;
  RebuildResult r;
  int rc = sync_piece(c, "ghf_crs_sync_piece", RebuildRequest{d_piece, piece_bytes, kSyncPiece, end_bit, first_bit}, nullptr, d_tree, &r);
  // with the tree's tables "end mark" can only mean: bits that are no code
  if (!rc && r.has_end_mark) rc = fail(c, GHF_E_CORRUPT, "the .crs body holds bits that are no code");
  *landing = r.landing;
  *n_symbols = rc ? 0 : r.n;
  return rc;
}

int ghf_crs_decode(ghf_ctx* c, const uint8_t* d_stream, size_t stream_bytes, int left_bits, const ghf_tree* d_tree,
                   const ghf_index* index, uint8_t* d_out, size_t cap, uint64_t* d_out_bytes) {
  if (!c || !d_stream || !d_tree || !d_out) return GHF_E_INVAL;
  if (!aligned16(d_stream)) return fail(c, GHF_E_INVAL, "d_stream must be 16-byte aligned");
  GHF_HIP(c, hipSetDevice(c->device));
  launch_crs_decode_tables(d_tree, c->d_dt, c->d_status, c->stream);
  c->prepared.forget();
  if (!index) {
    if (!c->rebuilt.describes(d_stream, stream_bytes)) {  // else: ghf_crs_decoded_size / ghf_crs_sync_piece did it
      RebuildRequest q;
      int rc = crs_request(c, d_stream, stream_bytes, left_bits, d_tree, &q);
      if (rc) return rc;
      if (q.end_bit == (uint64_t)q.hdr * 8) return nothing_decoded(c, d_out_bytes);
      q.cap = cap;
      rc = rebuild_index_at(c, q, nullptr);
      if (rc) return rc;
    }
    c->rebuilt.forget();
    index = &c->fidx;
    if (index->n_symbols == 0) return nothing_decoded(c, d_out_bytes);
  }
  DecParams p = {};
  p.stream = d_stream;
  p.stream_bytes = stream_bytes;
  p.no_end_mark = 1u;  // there is none in this format; the end of every segment but the last is checked against the side-car
  p.out = d_out;
  p.out_bytes = d_out_bytes;
  return decode_with_index(c, "ghf_crs_decode", index, cap, p);
}

}  // extern "C"
