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

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

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

}  // namespace

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

// ---------------------------------------------------------------------------------------------- batches
size_t ghf_compress_batch_bound(size_t max_item_bytes) { return ghf_compress_bound(max_item_bytes); }

int ghf_batch_index_alloc(ghf_ctx* c, uint32_t count, size_t max_item_bytes, ghf_batch_index* out) {
  if (!c || !out || max_item_bytes == 0 || max_item_bytes > GHF_BATCH_MAX_ITEM) return GHF_E_INVAL;
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

// the index covers `count` items of up to max_item_bytes, at the strides the kernels assume
static bool batch_index_covers(const ghf_batch_index* ix, uint32_t count, size_t max_item_bytes) {
  return ix->d_chunk_bit && ix->d_seg_bit && ix->count >= count && ix->max_item_bytes >= max_item_bytes &&
         ix->max_item_bytes <= GHF_BATCH_MAX_ITEM &&
         ix->blocks_per_item == blocks_for(ix->max_item_bytes) && ix->segs_per_item == segs_for(ix->max_item_bytes);
}

int ghf_compress_batch(ghf_ctx* c, const uint8_t* const* d_in_ptrs, const uint64_t* d_in_bytes, size_t max_item_bytes,
                       uint32_t count, uint8_t* const* d_out_ptrs, const uint64_t* d_out_caps, uint64_t* d_out_bytes,
                       ghf_code* d_codes, const ghf_batch_index* index, int* d_item_status) {
  if (!c) return GHF_E_INVAL;
  if (max_item_bytes == 0 || max_item_bytes > GHF_BATCH_MAX_ITEM)
    return fail(c, GHF_E_INVAL, "ghf_compress_batch: max_item_bytes must be 1 .. GHF_BATCH_MAX_ITEM");
  if (index && !batch_index_covers(index, count, max_item_bytes))
    return fail(c, GHF_E_INVAL, "ghf_compress_batch: index does not cover (count, max_item_bytes) (use ghf_batch_index_alloc)");
  if (count == 0) return GHF_OK;
  if (!d_in_ptrs || !d_in_bytes || !d_out_ptrs || !d_out_caps || !d_out_bytes || !d_item_status) return GHF_E_INVAL;
  GHF_HIP(c, hipSetDevice(c->device));
  if (!d_codes) {
    const int rc = grow(c, c->batch_codes, count);
    if (rc) return rc;
    d_codes = c->batch_codes.p;
  }
  BatchCompressParams p;
  p.in_ptrs = d_in_ptrs;
  p.in_bytes = d_in_bytes;
  p.max_item_bytes = max_item_bytes;
  p.out_ptrs = d_out_ptrs;
  p.out_caps = d_out_caps;
  p.out_bytes = d_out_bytes;
  p.codes = d_codes;
  p.chunk_bit = index ? index->d_chunk_bit : nullptr;
  p.seg_bit = index ? index->d_seg_bit : nullptr;
  p.blocks_per_item = index ? index->blocks_per_item : 0;
  p.segs_per_item = index ? index->segs_per_item : 0;
  p.item_status = d_item_status;
  launch_compress_batch(p, count, c->stream);
  GHF_HIP(c, hipGetLastError());
  return GHF_OK;
}

int ghf_decode_batch(ghf_ctx* c, const uint8_t* const* d_stream_ptrs, const uint64_t* d_stream_bytes, const ghf_code* d_codes,
                     const ghf_batch_index* index, const uint64_t* d_n_symbols, uint32_t count, uint8_t* const* d_out_ptrs,
                     const uint64_t* d_out_caps, uint64_t* d_out_bytes, int* d_item_status) {
  if (!c || !index) return GHF_E_INVAL;
  if (!batch_index_covers(index, count, 1))
    return fail(c, GHF_E_INVAL, "ghf_decode_batch: index does not cover count items (use ghf_batch_index_alloc)");
  if (count == 0) return GHF_OK;
  if (!d_stream_ptrs || !d_stream_bytes || !d_codes || !d_n_symbols || !d_out_ptrs || !d_out_caps || !d_out_bytes || !d_item_status)
    return GHF_E_INVAL;
  GHF_HIP(c, hipSetDevice(c->device));
  BatchDecodeParams p;
  p.stream_ptrs = d_stream_ptrs;
  p.stream_bytes = d_stream_bytes;
  p.codes = d_codes;
  p.chunk_bit = index->d_chunk_bit;
  p.seg_bit = index->d_seg_bit;
  p.blocks_per_item = index->blocks_per_item;
  p.segs_per_item = index->segs_per_item;
  p.max_item_bytes = index->max_item_bytes;
  p.n_symbols = d_n_symbols;
  p.out_ptrs = d_out_ptrs;
  p.out_caps = d_out_caps;
  p.out_bytes = d_out_bytes;
  p.item_status = d_item_status;
  launch_decode_batch(p, count, c->stream);
  GHF_HIP(c, hipGetLastError());
  return GHF_OK;
}

int ghf_decode_images_batch(ghf_ctx* c, const uint8_t* const* d_stream_ptrs, const uint64_t* d_stream_bytes, uint32_t count,
                            uint8_t* const* d_out_ptrs, const uint64_t* d_out_caps, uint64_t* d_out_bytes, ghf_code* d_codes,
                            int* d_item_status) {
  if (!c || !d_stream_ptrs || !d_stream_bytes || !d_out_bytes || !d_item_status) return GHF_E_INVAL;
  if (d_out_ptrs && !d_out_caps) return fail(c, GHF_E_INVAL, "ghf_decode_images_batch: d_out_ptrs without d_out_caps");
  if (count == 0) return GHF_OK;
  GHF_HIP(c, hipSetDevice(c->device));
  BatchImagesParams p;
  p.stream_ptrs = d_stream_ptrs;
  p.stream_bytes = d_stream_bytes;
  p.max_stream_bytes = ghf_compress_bound(GHF_BATCH_MAX_ITEM);
  p.out_ptrs = d_out_ptrs;
  p.out_caps = d_out_caps;
  p.out_bytes = d_out_bytes;
  p.codes = d_codes;
  p.item_status = d_item_status;
  p.stats = c->images_stats;
  launch_decode_images_batch(p, count, c->stream);
  GHF_HIP(c, hipGetLastError());
  return GHF_OK;
}

int ghf_decode_images_batch_stats(ghf_ctx* c, uint64_t* d_stats) {
  if (!c || (reinterpret_cast<uintptr_t>(d_stats) & 7u)) return GHF_E_INVAL;
  c->images_stats = d_stats;
  return GHF_OK;
}

// ---------------------------------------------------------------------------------------------- shared-code batches
int ghf_histogram_batch(ghf_ctx* c, const uint8_t* const* d_in_ptrs, const uint64_t* d_in_bytes, size_t max_item_bytes,
                        uint32_t count, unsigned flags, uint64_t* d_hist) {
  if (!c) return GHF_E_INVAL;
  if (max_item_bytes == 0 || max_item_bytes > GHF_BATCH_MAX_ITEM)
    return fail(c, GHF_E_INVAL, "ghf_histogram_batch: max_item_bytes must be 1 .. GHF_BATCH_MAX_ITEM");
  if (flags & ~GHF_HIST_COVER_ALL) return fail(c, GHF_E_INVAL, "ghf_histogram_batch: unknown flags");
  if (!d_in_ptrs || !d_in_bytes || !d_hist) return GHF_E_INVAL;
  if (count == 0) return GHF_OK;
  GHF_HIP(c, hipSetDevice(c->device));
  BatchHistParams p;
  p.in_ptrs = d_in_ptrs;
  p.in_bytes = d_in_bytes;
  p.max_item_bytes = max_item_bytes;
  p.count = count;
  p.hist = d_hist;
  launch_histogram_batch(p, flags, c->stream);
  GHF_HIP(c, hipGetLastError());
  return GHF_OK;
}

size_t ghf_compress_batch_shared_bound(size_t max_item_bytes) { return (4 * max_item_bytes + 4 + 15) & ~(size_t)15; }

int ghf_compress_batch_shared(ghf_ctx* c, const uint8_t* const* d_in_ptrs, const uint64_t* d_in_bytes, size_t max_item_bytes,
                              uint32_t count, const ghf_code* d_code, uint8_t* const* d_out_ptrs, const uint64_t* d_out_caps,
                              uint64_t* d_out_bytes, const ghf_batch_index* index, int* d_item_status) {
  if (!c) return GHF_E_INVAL;
  if (max_item_bytes == 0 || max_item_bytes > GHF_BATCH_MAX_ITEM)
    return fail(c, GHF_E_INVAL, "ghf_compress_batch_shared: max_item_bytes must be 1 .. GHF_BATCH_MAX_ITEM");
  if (index && !batch_index_covers(index, count, max_item_bytes))
    return fail(c, GHF_E_INVAL, "ghf_compress_batch_shared: index does not cover (count, max_item_bytes) (use ghf_batch_index_alloc)");
  if (!d_code || !aligned16(d_code)) return fail(c, GHF_E_INVAL, "ghf_compress_batch_shared: d_code is null or not 16-byte aligned");
  if (!d_in_ptrs || !d_in_bytes || !d_out_ptrs || !d_out_caps || !d_out_bytes || !d_item_status) return GHF_E_INVAL;
  if (count == 0) return GHF_OK;
  GHF_HIP(c, hipSetDevice(c->device));
  BatchSharedCompressParams p;
  p.in_ptrs = d_in_ptrs;
  p.in_bytes = d_in_bytes;
  p.max_item_bytes = max_item_bytes;
  p.code = d_code;
  p.out_ptrs = d_out_ptrs;
  p.out_caps = d_out_caps;
  p.out_bytes = d_out_bytes;
  p.chunk_bit = index ? index->d_chunk_bit : nullptr;
  p.seg_bit = index ? index->d_seg_bit : nullptr;
  p.blocks_per_item = index ? index->blocks_per_item : 0;
  p.segs_per_item = index ? index->segs_per_item : 0;
  p.item_status = d_item_status;
  launch_compress_batch_shared(p, count, c->stream);
  GHF_HIP(c, hipGetLastError());
  return GHF_OK;
}

int ghf_decode_batch_shared(ghf_ctx* c, const uint8_t* const* d_stream_ptrs, const uint64_t* d_stream_bytes, const ghf_code* d_code,
                            const ghf_batch_index* index, const uint64_t* d_n_symbols, uint32_t count, uint8_t* const* d_out_ptrs,
                            const uint64_t* d_out_caps, uint64_t* d_out_bytes, int* d_item_status) {
  if (!c || !index) return GHF_E_INVAL;
  if (!batch_index_covers(index, count, 1))
    return fail(c, GHF_E_INVAL, "ghf_decode_batch_shared: index does not cover count items (use ghf_batch_index_alloc)");
  if (!d_code || !aligned16(d_code)) return fail(c, GHF_E_INVAL, "ghf_decode_batch_shared: d_code is null or not 16-byte aligned");
  if (!d_stream_ptrs || !d_stream_bytes || !d_n_symbols || !d_out_ptrs || !d_out_caps || !d_out_bytes || !d_item_status)
    return GHF_E_INVAL;
  if (count == 0) return GHF_OK;
  GHF_HIP(c, hipSetDevice(c->device));
  BatchSharedDecodeParams p;
  p.stream_ptrs = d_stream_ptrs;
  p.stream_bytes = d_stream_bytes;
  p.code = d_code;
  p.chunk_bit = index->d_chunk_bit;
  p.seg_bit = index->d_seg_bit;
  p.blocks_per_item = index->blocks_per_item;
  p.segs_per_item = index->segs_per_item;
  p.max_item_bytes = index->max_item_bytes;
  p.n_symbols = d_n_symbols;
  p.out_ptrs = d_out_ptrs;
  p.out_caps = d_out_caps;
  p.out_bytes = d_out_bytes;
  p.item_status = d_item_status;
  launch_decode_batch_shared(p, count, c->stream);
  GHF_HIP(c, hipGetLastError());
  return GHF_OK;
}

int ghf_decode_bodies_batch_shared(ghf_ctx* c, const uint8_t* const* d_stream_ptrs, const uint64_t* d_stream_bytes,
                                   const ghf_code* d_code, uint32_t count, uint8_t* const* d_out_ptrs, const uint64_t* d_out_caps,
                                   uint64_t* d_out_bytes, int* d_item_status) {
  if (!c || !d_stream_ptrs || !d_stream_bytes || !d_out_bytes || !d_item_status) return GHF_E_INVAL;
  if (d_out_ptrs && !d_out_caps) return fail(c, GHF_E_INVAL, "ghf_decode_bodies_batch_shared: d_out_ptrs without d_out_caps");
  if (!d_code || !aligned16(d_code)) return fail(c, GHF_E_INVAL, "ghf_decode_bodies_batch_shared: d_code is null or not 16-byte aligned");
  if (count == 0) return GHF_OK;
  GHF_HIP(c, hipSetDevice(c->device));
  BatchSharedBodiesParams p;
  p.stream_ptrs = d_stream_ptrs;
  p.stream_bytes = d_stream_bytes;
  p.max_stream_bytes = ghf_compress_batch_shared_bound(GHF_BATCH_MAX_ITEM);
  p.code = d_code;
  p.out_ptrs = d_out_ptrs;
  p.out_caps = d_out_caps;
  p.out_bytes = d_out_bytes;
  p.item_status = d_item_status;
  p.stats = c->images_stats;
  launch_decode_bodies_batch_shared(p, count, c->stream);
  GHF_HIP(c, hipGetLastError());
  return GHF_OK;
}

// ---------------------------------------------------------------------------------------------- shared-code batches of byte planes
static inline bool planes_elem_ok(uint32_t elem_bytes) { return elem_bytes == 2 || elem_bytes == 4 || elem_bytes == 8; }
// max_item_bytes of a batch of elements: 1 .. GHF_BATCH_MAX_ITEM and a whole number of elements
static inline bool planes_item_ok(size_t max_item_bytes, uint32_t elem_bytes) {
  return max_item_bytes != 0 && max_item_bytes <= GHF_BATCH_MAX_ITEM && max_item_bytes % elem_bytes == 0;
}

int ghf_histogram_batch_planes(ghf_ctx* c, const uint8_t* const* d_in_ptrs, const uint64_t* d_in_bytes, size_t max_item_bytes,
                               uint32_t count, uint32_t elem_bytes, unsigned flags, uint64_t* d_hists) {
  if (!c) return GHF_E_INVAL;
  if (!planes_elem_ok(elem_bytes)) return fail(c, GHF_E_INVAL, "ghf_histogram_batch_planes: elem_bytes must be 2, 4 or 8");
  if (!planes_item_ok(max_item_bytes, elem_bytes))
    return fail(c, GHF_E_INVAL, "ghf_histogram_batch_planes: max_item_bytes must be 1 .. GHF_BATCH_MAX_ITEM and a multiple of elem_bytes");
  if (flags & ~GHF_HIST_COVER_ALL) return fail(c, GHF_E_INVAL, "ghf_histogram_batch_planes: unknown flags");
  if (!d_in_ptrs || !d_in_bytes || !d_hists) return GHF_E_INVAL;
  if (count == 0) return GHF_OK;
  GHF_HIP(c, hipSetDevice(c->device));
  BatchPlanesHistParams p;
  p.in_ptrs = d_in_ptrs;
  p.in_bytes = d_in_bytes;
  p.max_item_bytes = max_item_bytes;
  p.count = count;
  p.hists = d_hists;
  launch_histogram_batch_planes(p, elem_bytes, flags, c->stream);
  GHF_HIP(c, hipGetLastError());
  return GHF_OK;
}

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

size_t ghf_compress_batch_planes_shared_bound(size_t max_item_bytes, uint32_t elem_bytes) {
  return planes_elem_ok(elem_bytes) ? ghf_compress_batch_shared_bound(max_item_bytes / elem_bytes) : 0;
}

// the index covers count * elem_bytes slots of max_item_bytes / elem_bytes symbols (the product fits: count is 32 bits wide)
static bool planes_index_covers(const ghf_batch_index* ix, uint32_t count, uint32_t elem_bytes, size_t plane_symbols) {
  return (uint64_t)count * elem_bytes <= 0xFFFFFFFFull && batch_index_covers(ix, count * elem_bytes, plane_symbols);
}

int ghf_compress_batch_planes_shared(ghf_ctx* c, const uint8_t* const* d_in_ptrs, const uint64_t* d_in_bytes, size_t max_item_bytes,
                                     uint32_t count, uint32_t elem_bytes, const ghf_code* d_codes, uint8_t* const* d_out_ptrs,
                                     const uint64_t* d_out_caps, uint64_t* d_out_bytes, const ghf_batch_index* index,
                                     int* d_item_status) {
  if (!c) return GHF_E_INVAL;
  if (!planes_elem_ok(elem_bytes)) return fail(c, GHF_E_INVAL, "ghf_compress_batch_planes_shared: elem_bytes must be 2, 4 or 8");
  if (!planes_item_ok(max_item_bytes, elem_bytes))
    return fail(c, GHF_E_INVAL, "ghf_compress_batch_planes_shared: max_item_bytes must be 1 .. GHF_BATCH_MAX_ITEM and a multiple of elem_bytes");
  if ((uint64_t)count * elem_bytes > 0xFFFFFFFFull) return fail(c, GHF_E_INVAL, "ghf_compress_batch_planes_shared: count * elem_bytes beyond 32 bits");
  if (index && !planes_index_covers(index, count, elem_bytes, max_item_bytes / elem_bytes))
    return fail(c, GHF_E_INVAL, "ghf_compress_batch_planes_shared: index does not cover (count * elem_bytes, max_item_bytes / elem_bytes)");
  if (!d_codes || !aligned16(d_codes)) return fail(c, GHF_E_INVAL, "ghf_compress_batch_planes_shared: d_codes is null or not 16-byte aligned");
  if (!d_in_ptrs || !d_in_bytes || !d_out_ptrs || !d_out_caps || !d_out_bytes || !d_item_status) return GHF_E_INVAL;
  if (count == 0) return GHF_OK;
  GHF_HIP(c, hipSetDevice(c->device));
  BatchPlanesCompressParams p;
  p.in_ptrs = d_in_ptrs;
  p.in_bytes = d_in_bytes;
  p.max_item_bytes = max_item_bytes;
  p.codes = d_codes;
  p.out_ptrs = d_out_ptrs;
  p.out_caps = d_out_caps;
  p.out_bytes = d_out_bytes;
  p.chunk_bit = index ? index->d_chunk_bit : nullptr;
  p.seg_bit = index ? index->d_seg_bit : nullptr;
  p.blocks_per_item = index ? index->blocks_per_item : 0;
  p.segs_per_item = index ? index->segs_per_item : 0;
  p.item_status = d_item_status;
  launch_compress_batch_planes_shared(p, count, elem_bytes, c->stream);
  GHF_HIP(c, hipGetLastError());
  return GHF_OK;
}

int ghf_decode_batch_planes_shared(ghf_ctx* c, const uint8_t* const* d_stream_ptrs, const uint64_t* d_stream_bytes,
                                   const ghf_code* d_codes, const ghf_batch_index* index, const uint64_t* d_n_elems, uint32_t count,
                                   uint32_t elem_bytes, uint8_t* const* d_out_ptrs, const uint64_t* d_out_caps, uint64_t* d_out_bytes,
                                   int* d_item_status) {
  if (!c || !index) return GHF_E_INVAL;
  if (!planes_elem_ok(elem_bytes)) return fail(c, GHF_E_INVAL, "ghf_decode_batch_planes_shared: elem_bytes must be 2, 4 or 8");
  if (!planes_index_covers(index, count, elem_bytes, 1))
    return fail(c, GHF_E_INVAL, "ghf_decode_batch_planes_shared: index does not cover count * elem_bytes slots");
  if (!d_codes || !aligned16(d_codes)) return fail(c, GHF_E_INVAL, "ghf_decode_batch_planes_shared: d_codes is null or not 16-byte aligned");
  if (!d_stream_ptrs || !d_stream_bytes || !d_n_elems || !d_out_ptrs || !d_out_caps || !d_out_bytes || !d_item_status)
    return GHF_E_INVAL;
  if (count == 0) return GHF_OK;
  GHF_HIP(c, hipSetDevice(c->device));
  BatchPlanesDecodeParams p;
  p.stream_ptrs = d_stream_ptrs;
  p.stream_bytes = d_stream_bytes;
  p.codes = d_codes;
  p.chunk_bit = index->d_chunk_bit;
  p.seg_bit = index->d_seg_bit;
  p.blocks_per_item = index->blocks_per_item;
  p.segs_per_item = index->segs_per_item;
  p.max_plane_symbols = index->max_item_bytes;
  p.n_elems = d_n_elems;
  p.out_ptrs = d_out_ptrs;
  p.out_caps = d_out_caps;
  p.out_bytes = d_out_bytes;
  p.item_status = d_item_status;
  launch_decode_batch_planes_shared(p, count, elem_bytes, c->stream);
  GHF_HIP(c, hipGetLastError());
  return GHF_OK;
}

int ghf_decode_bodies_batch_planes_shared(ghf_ctx* c, const uint8_t* const* d_stream_ptrs, const uint64_t* d_stream_bytes,
                                          const ghf_code* d_codes, uint32_t count, uint32_t elem_bytes, uint8_t* const* d_out_ptrs,
                                          const uint64_t* d_out_caps, uint64_t* d_out_bytes, int* d_item_status) {
  if (!c || !d_stream_ptrs || !d_stream_bytes || !d_out_bytes || !d_item_status) return GHF_E_INVAL;
  if (!planes_elem_ok(elem_bytes)) return fail(c, GHF_E_INVAL, "ghf_decode_bodies_batch_planes_shared: elem_bytes must be 2, 4 or 8");
  if (d_out_ptrs && !d_out_caps) return fail(c, GHF_E_INVAL, "ghf_decode_bodies_batch_planes_shared: d_out_ptrs without d_out_caps");
  if (!d_codes || !aligned16(d_codes))
    return fail(c, GHF_E_INVAL, "ghf_decode_bodies_batch_planes_shared: d_codes is null or not 16-byte aligned");
  if (count == 0) return GHF_OK;
  GHF_HIP(c, hipSetDevice(c->device));
  BatchPlanesBodiesParams p;
  p.stream_ptrs = d_stream_ptrs;
  p.stream_bytes = d_stream_bytes;
  p.max_stream_bytes = ghf_compress_batch_shared_bound(GHF_BATCH_MAX_ITEM);
  p.codes = d_codes;
  p.out_ptrs = d_out_ptrs;
  p.out_caps = d_out_caps;
  p.out_bytes = d_out_bytes;
  p.item_status = d_item_status;
  p.stats = c->images_stats;
  launch_decode_bodies_batch_planes_shared(p, count, elem_bytes, c->stream);
  GHF_HIP(c, hipGetLastError());
  return GHF_OK;
}

// ---------------------------------------------------------------------------------------------- stored shared-code bodies
size_t ghf_batch_seek_bytes(size_t n_symbols) { return (size_t)batch_seek_bytes_for(n_symbols); }
size_t ghf_batch_seek_bound(size_t max_item_bytes) { return (ghf_batch_seek_bytes(max_item_bytes) + 15) & ~(size_t)15; }

int ghf_batch_seek_pack(ghf_ctx* c, const ghf_batch_index* index, const uint64_t* d_in_bytes, uint32_t count, uint32_t elem_bytes,
                        uint8_t* const* d_rec_ptrs, const uint64_t* d_rec_caps, uint64_t* d_rec_bytes, int* d_slot_status) {
  if (!c || !index) return GHF_E_INVAL;
  if (elem_bytes != 1 && !planes_elem_ok(elem_bytes)) return fail(c, GHF_E_INVAL, "ghf_batch_seek_pack: elem_bytes must be 1, 2, 4 or 8");
  if (!planes_index_covers(index, count, elem_bytes, 1))
    return fail(c, GHF_E_INVAL, "ghf_batch_seek_pack: index does not cover count * elem_bytes slots (use ghf_batch_index_alloc)");
  if (!d_in_bytes || !d_rec_ptrs || !d_rec_caps || !d_rec_bytes || !d_slot_status) return GHF_E_INVAL;
  if (count == 0) return GHF_OK;
  GHF_HIP(c, hipSetDevice(c->device));
  BatchSeekPackParams p;
  p.chunk_bit = index->d_chunk_bit;
  p.seg_bit = index->d_seg_bit;
  p.blocks_per_item = index->blocks_per_item;
  p.segs_per_item = index->segs_per_item;
  p.max_slice_symbols = index->max_item_bytes;
  p.in_bytes = d_in_bytes;
  p.elem_bytes = elem_bytes;
  p.rec_ptrs = d_rec_ptrs;
  p.rec_caps = d_rec_caps;
  p.rec_bytes = d_rec_bytes;
  p.slot_status = d_slot_status;
  launch_batch_seek_pack(p, count * elem_bytes, c->stream);
  GHF_HIP(c, hipGetLastError());
  return GHF_OK;
}

// the two decoders of stored bodies: elem_bytes = 1 is the flat call
static int decode_bodies_batch_seek(ghf_ctx* c, const char* who, const uint8_t* const* d_stream_ptrs, const uint64_t* d_stream_bytes,
                                    const uint8_t* const* d_rec_ptrs, const uint64_t* d_rec_bytes, const ghf_code* d_codes, uint32_t count,
                                    uint32_t elem_bytes, uint8_t* const* d_out_ptrs, const uint64_t* d_out_caps, uint64_t* d_out_bytes,
                                    int* d_item_status) {
  if (!c || !d_stream_ptrs || !d_stream_bytes || !d_rec_ptrs || !d_rec_bytes || !d_out_bytes || !d_item_status) return GHF_E_INVAL;
  if (elem_bytes != 1 && !planes_elem_ok(elem_bytes)) return fail(c, GHF_E_INVAL, (std::string(who) + ": elem_bytes must be 2, 4 or 8").c_str());
  if (d_out_ptrs && !d_out_caps) return fail(c, GHF_E_INVAL, (std::string(who) + ": d_out_ptrs without d_out_caps").c_str());
  if (!d_codes || !aligned16(d_codes)) return fail(c, GHF_E_INVAL, (std::string(who) + ": the code array is null or not 16-byte aligned").c_str());
  if (count == 0) return GHF_OK;
  GHF_HIP(c, hipSetDevice(c->device));
  BatchSeekDecodeParams p;
  p.stream_ptrs = d_stream_ptrs;
  p.stream_bytes = d_stream_bytes;
  p.rec_ptrs = d_rec_ptrs;
  p.rec_bytes = d_rec_bytes;
  p.max_stream_bytes = ghf_compress_batch_shared_bound(GHF_BATCH_MAX_ITEM);
  p.codes = d_codes;
  p.out_ptrs = d_out_ptrs;
  p.out_caps = d_out_caps;
  p.out_bytes = d_out_bytes;
  p.item_status = d_item_status;
  launch_decode_bodies_batch_seek(p, count, elem_bytes, c->stream);
  GHF_HIP(c, hipGetLastError());
  return GHF_OK;
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
  if (c && !planes_elem_ok(elem_bytes))
    return fail(c, GHF_E_INVAL, "ghf_decode_bodies_batch_planes_shared_seek: elem_bytes must be 2, 4 or 8");
  return decode_bodies_batch_seek(c, "ghf_decode_bodies_batch_planes_shared_seek", d_stream_ptrs, d_stream_bytes, d_rec_ptrs, d_rec_bytes,
                                  d_codes, count, elem_bytes, d_out_ptrs, d_out_caps, d_out_bytes, d_item_status);
}

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

// ---------------------------------------------------------------------------------------------- byte planes
// (no reference counterpart)
size_t ghf_planes_slot_bytes(size_t n_elems) { return (ghf_compress_bound(n_elems) + 15) & ~(size_t)15; }

static inline bool elem_bytes_ok(uint32_t e) { return e == 2 || e == 4 || e == 8; }
static inline bool elems_overflow(size_t n_elems, uint32_t e) { return n_elems > (size_t)-1 / e; }
// ... and for the calls that go through the workspace, whose planes sit at n_elems rounded up to 256
static inline bool workspace_overflow(size_t n_elems, uint32_t e) { return elems_overflow(n_elems, e) || elems_overflow(n_elems + 255, e); }

// The calls against a base share the implementation of their plain calls: a Base says whether the
// call has one, and d_base is null exactly where it has none -- which is what selects the plain kernels in the launchers.
// A delta call with a null or misaligned d_base is refused where the other pointers are.
struct Base {
  bool delta;
  const uint8_t* p;
  bool null() const { return delta && !p; }
  bool misaligned() const { return delta && !aligned16(p); }
};
static inline Base no_base() { return {false, nullptr}; }
static inline Base base_of(const uint8_t* d_base) { return {true, d_base}; }

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
  GHF_HIP(c, hipSetDevice(c->device));
  launch_planes_split(d_in, base.p, n_elems, elem_bytes, d_planes, plane_stride, c->stream);
  GHF_HIP(c, hipGetLastError());
  return GHF_OK;
}
int ghf_planes_split(ghf_ctx* c, const uint8_t* d_in, size_t n_elems, uint32_t elem_bytes, uint8_t* d_planes, size_t plane_stride) {
  return planes_split(c, "ghf_planes_split", d_in, no_base(), n_elems, elem_bytes, d_planes, plane_stride);
}

static int planes_merge(ghf_ctx* c, const char* who, const uint8_t* d_planes, size_t plane_stride, Base base, size_t n_elems,
                        uint32_t elem_bytes, uint8_t* d_out) {
  const int rc = planes_args(c, who, d_out, d_planes, plane_stride, n_elems, elem_bytes, base);
  if (rc) return rc;
  GHF_HIP(c, hipSetDevice(c->device));
  launch_planes_merge(d_planes, plane_stride, base.p, n_elems, elem_bytes, d_out, nullptr, c->stream);
  GHF_HIP(c, hipGetLastError());
  return GHF_OK;
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
  GHF_HIP(c, hipSetDevice(c->device));
  launch_planes_merge_range(d_planes, plane_stride, base.p, first, count, elem_bytes, d_out, nullptr, c->stream);
  GHF_HIP(c, hipGetLastError());
  return GHF_OK;
}
int ghf_planes_merge_range(ghf_ctx* c, const uint8_t* d_planes, size_t plane_stride, size_t first, size_t count, uint32_t elem_bytes,
                           uint8_t* d_out) {
  return planes_merge_range(c, "ghf_planes_merge_range", d_planes, plane_stride, no_base(), first, count, elem_bytes, d_out);
}

// the context's plane workspace for n_elems elements (workspace_overflow has cleared them): *stride <- the distance
// between two planes
static int planes_workspace(ghf_ctx* c, size_t n_elems, uint32_t elem_bytes, size_t* stride) {
  *stride = (n_elems + 255) & ~(size_t)255;
  return grow(c, c->planes, *stride * elem_bytes);
}

int ghf_compress_planes(ghf_ctx* c, const uint8_t* d_in, size_t n_elems, uint32_t elem_bytes, uint8_t* d_out, size_t slot_bytes,
                        uint64_t* d_out_bytes, ghf_code* d_codes, const ghf_index* indexes) {
  if (!c || !d_in || !d_out || !d_out_bytes) return GHF_E_INVAL;
  if (!elem_bytes_ok(elem_bytes)) return fail(c, GHF_E_INVAL, "ghf_compress_planes: elem_bytes must be 2, 4 or 8");
  if (!aligned16(d_in) || !aligned16(d_out) || (slot_bytes & 15u))
    return fail(c, GHF_E_INVAL, "ghf_compress_planes: d_in, d_out and slot_bytes must be multiples of 16");
  if (workspace_overflow(n_elems, elem_bytes)) return fail(c, GHF_E_INVAL, "ghf_compress_planes: n_elems * elem_bytes overflows");
  for (uint32_t p = 0; indexes && p < elem_bytes; ++p)
    if (indexes[p].n_symbols != n_elems || !index_has_arrays(&indexes[p]))
      return fail(c, GHF_E_INVAL, "ghf_compress_planes: an index does not match n_elems (use ghf_index_alloc)");
  if (n_elems == 0) return fail(c, GHF_E_EMPTY, "ghf_compress_planes: no elements");
  if (slot_bytes < ghf_planes_slot_bytes(n_elems)) return fail(c, GHF_E_CAP, "ghf_compress_planes: slot_bytes below ghf_planes_slot_bytes(n_elems)");
  GHF_HIP(c, hipSetDevice(c->device));
  size_t stride = 0;
  int rc = planes_workspace(c, n_elems, elem_bytes, &stride);
  if (rc) return rc;
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
// k_histogram_planes and its finish on the stream.  The finish is what leaves the replicas zero for the next call: if it
// cannot be queued behind a counting launch that was, a memset takes its place before the error is returned
static int histogram_planes_into(ghf_ctx* c, const char* who, const uint8_t* d_in, const uint8_t* d_base, size_t n_elems,
                                 uint32_t elem_bytes, unsigned flags, uint64_t* d_hists) {
  const hipError_t e = launch_histogram_planes(d_in, d_base, n_elems, elem_bytes, flags, c->d_planes_hist_acc, d_hists, c->stream);
  if (e == hipSuccess) return GHF_OK;
  (void)hipMemsetAsync(c->d_planes_hist_acc, 0, kPlanesHistAccWords * sizeof(uint64_t), c->stream);
  return fail(c, GHF_E_HIP, who, e);
}

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
  GHF_HIP(c, hipSetDevice(c->device));
  launch_planes_image_bytes(d_hists, d_codes, elem_bytes, d_bytes, c->stream);
  GHF_HIP(c, hipGetLastError());
  return GHF_OK;
}

static int compress_planes_coded(ghf_ctx* c, const char* who, const uint8_t* d_in, Base base, size_t n_elems, uint32_t elem_bytes,
                                 ghf_code* d_codes, unsigned flags, uint8_t* d_out, size_t slot_bytes, uint64_t* d_out_bytes,
                                 const ghf_index* indexes) {
  if (!c || !d_in || !d_out || !d_out_bytes || !d_codes || base.null()) return GHF_E_INVAL;
  const std::string f = std::string(who) + ": ";
  if (!elem_bytes_ok(elem_bytes)) return fail(c, GHF_E_INVAL, (f + "elem_bytes must be 2, 4 or 8").c_str());
  if (!aligned16(d_in) || !aligned16(d_out) || (slot_bytes & 15u) || !aligned16(d_codes) || base.misaligned())
    return fail(c, GHF_E_INVAL, (f + "d_in, d_base, d_out, d_codes and slot_bytes must be multiples of 16").c_str());
  if (flags & ~GHF_PLANES_BUILD_CODES) return fail(c, GHF_E_INVAL, (f + "unknown flags").c_str());
  if (workspace_overflow(n_elems, elem_bytes)) return fail(c, GHF_E_INVAL, (f + "n_elems * elem_bytes overflows").c_str());
  for (uint32_t p = 0; indexes && p < elem_bytes; ++p)
    if (indexes[p].n_symbols != n_elems || !index_has_arrays(&indexes[p]))
      return fail(c, GHF_E_INVAL, (f + "an index does not match n_elems (use ghf_index_alloc)").c_str());
  if (n_elems == 0) return fail(c, GHF_E_EMPTY, (f + "no elements").c_str());
  if (slot_bytes < ghf_planes_slot_bytes(n_elems)) return fail(c, GHF_E_CAP, (f + "slot_bytes below ghf_planes_slot_bytes(n_elems)").c_str());
  GHF_HIP(c, hipSetDevice(c->device));
  size_t stride = 0;
  int rc = planes_workspace(c, n_elems, elem_bytes, &stride);
  if (rc) return rc;
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
  // K1 has not seen these planes: whatever it remembers about an address inside the workspace is of another call, and the
  // planner counts each plane itself (k_chunk_bits_direct)
  c->hist.forget();
  for (uint32_t p = 0; p < elem_bytes && !rc; ++p) {  // compressor.h:70-72, once per plane: what ghf_compress_ex does behind its code build
    const uint8_t* plane = c->planes.p + p * stride;
    if ((rc = ghf_encode_plan(c, plane, n_elems, d_codes + p, &c->d->total_bits))) break;
    if ((rc = ghf_encode_emit(c, plane, n_elems, d_codes + p, nullptr, GHF_EMIT_LAST | GHF_EMIT_HEADER, d_out + p * slot_bytes, slot_bytes,
                              indexes ? indexes + p : nullptr, c->d->end)))
      break;
    launch_store_u64(d_out_bytes + p, &c->d->end[1], 0, c->stream);
    GHF_HIP(c, hipGetLastError());
  }
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
  for (uint32_t p = 0; p < elem_bytes; ++p) {
    if (!indexes) {  // the side-car-less path: synchronises, and keeps the side-car for the decode that follows
      uint64_t n_p = 0;
      if ((rc = ghf_decoded_size(c, h_stream_ptrs[p], h_stream_bytes[p], d_codes + p, &n_p))) return rc;
      if (n_p != n_elems) return fail(c, GHF_E_CORRUPT, (f + "a plane does not decode to n_elems bytes").c_str());
    }
    if ((rc = ghf_decode(c, h_stream_ptrs[p], h_stream_bytes[p], d_codes + p, indexes ? indexes + p : nullptr, c->planes.p + p * stride,
                         stride, nullptr)))
      return rc;
  }
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

// ---------------------------------------------------------------------------------------------- seek table
// (no reference counterpart; the format: DESIGN.md "Seekable .crs2")
size_t ghf_seek_bytes(size_t n_symbols) { return kSeekHeaderBytes + kSeekRecordBytes * (size_t)blocks_for(n_symbols); }

static inline uint32_t le32(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
static inline uint64_t le64(const uint8_t* p) { return (uint64_t)le32(p) | ((uint64_t)le32(p + 4) << 32); }

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

// the part of "this info describes a table of table_bytes" that every consumer of (info, d_table) asks for
static int seek_table_ok(ghf_ctx* c, const char* who, const ghf_seek_info* info, const uint8_t* d_table, size_t table_bytes) {
  const std::string f = std::string(who) + ": ";
  if (!aligned16(d_table)) return fail(c, GHF_E_INVAL, (f + "d_table must be 16-byte aligned").c_str());
  if (info->version != kSeekVersion || (info->flags & ~(uint32_t)GHF_INDEX_NO_END_MARK) || info->n_blocks != blocks_for(info->n_symbols) ||
      info->n_blocks >= kDecMaxGroups || table_bytes != ghf_seek_bytes(info->n_symbols))
    return fail(c, GHF_E_FORMAT, (f + "the seek table does not have the size its header implies").c_str());
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
  SeekExpandParams p = {};
  p.records = d_table + kSeekHeaderBytes;
  p.stream = d_stream;
  p.stream_bytes = stream_bytes;
  p.dt = c->d_dt;
  p.n_symbols = info->n_symbols;
  p.n_blocks = info->n_blocks;
  p.g0 = g0;
  p.g1 = g1;
  p.chunk_bit = d_chunk_bit;
  p.seg_bit = d_seg_bit;
  p.status = c->d_status;
  launch_seek_expand(p, c->stream);
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
  if (end > gI * kBlockSymbols) {
    // K7 on a view of the side-car that begins at block gI and ends with the range: a segment's start depends on its own
    // block only.  The view's last segment may be cut short by the range; only the stream's own end is followed by the end mark.
    DecParams p = {};
    p.stream = d_stream;
    p.stream_bytes = stream_bytes;
    p.dt = c->d_dt;
    p.chunk_bit = chunk_bit + (gI - gA);
    p.seg_bit = seg_bit + (gI - gA) * (kBlockSymbols / kSegSymbols);
    p.n_symbols = end - gI * kBlockSymbols;
    p.n_segs = segs_for(p.n_symbols);
    p.no_end_mark = (end == n && !(flags & GHF_INDEX_NO_END_MARK)) ? 0u : 1u;
    p.out = d_out + (gI * kBlockSymbols - first);
    p.out_bytes = nullptr;
    p.status = c->d_status;
    launch_decode(p, c->stream);
  }
  GHF_HIP(c, hipGetLastError());
  return GHF_OK;
}

// ---------------------------------------------------------------------------------------------- element range of byte planes
// (no reference counterpart)
static int decode_planes_range(ghf_ctx* c, const char* who, const uint8_t* const* h_stream_ptrs, const size_t* h_stream_bytes,
                               const ghf_code* d_codes, const ghf_index* indexes, const ghf_seek_info* h_infos,
                               const uint8_t* const* h_table_ptrs, const size_t* h_table_bytes, Base base, uint32_t elem_bytes,
                               uint64_t first, uint64_t count, uint8_t* d_out, size_t cap) {
  if (!c || !h_stream_ptrs || !h_stream_bytes || !d_codes || !d_out || base.null()) return GHF_E_INVAL;
  const std::string f = std::string(who) + ": ";
  if (!elem_bytes_ok(elem_bytes)) return fail(c, GHF_E_INVAL, (f + "elem_bytes must be 2, 4 or 8").c_str());
  const bool by_table = h_infos || h_table_ptrs || h_table_bytes;
  if ((indexes != nullptr) == by_table || (by_table && !(h_infos && h_table_ptrs && h_table_bytes)))
    return fail(c, GHF_E_INVAL, (f + "exactly one of indexes / (h_infos, h_table_ptrs, h_table_bytes) must be given").c_str());
  for (uint32_t p = 0; p < elem_bytes; ++p) {
    if (!h_stream_ptrs[p] || !aligned16(h_stream_ptrs[p]))
      return fail(c, GHF_E_INVAL, (f + "a stream pointer is null or not 16-byte aligned").c_str());
    if (by_table && (!h_table_ptrs[p] || !aligned16(h_table_ptrs[p])))
      return fail(c, GHF_E_INVAL, (f + "a table pointer is null or not 16-byte aligned").c_str());
  }
  if (!aligned16(d_out) || base.misaligned()) return fail(c, GHF_E_INVAL, (f + "d_out and d_base must be 16-byte aligned").c_str());
  const uint64_t n_elems = by_table ? h_infos[0].n_symbols : indexes[0].n_symbols;
  for (uint32_t p = 0; p < elem_bytes; ++p) {
    if (!by_table && indexes[p].n_symbols != 0 && !index_is_whole(&indexes[p]))
      return fail(c, GHF_E_INVAL, (f + "malformed index").c_str());
    if ((by_table ? h_infos[p].n_symbols : indexes[p].n_symbols) != n_elems)
      return fail(c, GHF_E_INVAL, (f + "the planes disagree on n_symbols").c_str());
  }
  if (first > n_elems || count > n_elems - first) return fail(c, GHF_E_INVAL, (f + "first + count exceeds n_elems").c_str());
  // the workspace holds the range from the start of its first block (below), and a vector more for the merge's second load
  const size_t lead = (size_t)(first % kBlockSymbols);
  if (count > (size_t)-1 - lead - 16 || workspace_overflow((size_t)count + lead + 16, elem_bytes))
    return fail(c, GHF_E_INVAL, (f + "count * elem_bytes overflows").c_str());
  for (uint32_t p = 0; by_table && p < elem_bytes; ++p) {  // every plane before anything is queued for the first
    const int rc = seek_table_ok(c, who, h_infos + p, h_table_ptrs[p], h_table_bytes[p]);
    if (rc) return rc;
  }
  if (cap < count * elem_bytes) return fail(c, GHF_E_CAP, (f + "output capacity below count * elem_bytes").c_str());
  if (count == 0) return GHF_OK;
  GHF_HIP(c, hipSetDevice(c->device));
  // Every plane is decoded from the start of the block that holds `first`: plane p's byte `first - lead` lands on the
  // 16-byte aligned start of its workspace plane, so every later byte sits at an address congruent to its index modulo 16 --
  // what K7's 16-byte store path asks for -- and no block is entered in its middle: ghf_decode_range queues no k_decode_head,
  // whose one wave walks up to a block serially (DESIGN.md section 17 has the measurement).  The up to 4095 symbols in front
  // of the range are one K7 block of work; the merge skips them and takes the skew out.
  size_t stride = 0;
  int rc = planes_workspace(c, (size_t)count + lead + 16, elem_bytes, &stride);
  if (rc) return rc;
  const uint64_t from = first - lead, end = first + count;
  if (!by_table) {
    for (uint32_t p = 0; p < elem_bytes; ++p)
      if ((rc = ghf_decode_range(c, h_stream_ptrs[p], h_stream_bytes[p], d_codes + p, indexes + p, nullptr, nullptr, 0, from, end - from,
                                 c->planes.p + p * stride, stride)))
        return rc;
  } else {
    // From tables ghf_decode_range would expand every plane by itself, and k_seek_expand has a latency floor -- a lane walks
    // its 512 symbols serially -- that a range does not shrink: E floors one after the other cost more than decoding the
    // whole tensor from side-cars.  So: all E table sets first, ONE launch that expands the covered blocks of all planes
    // (k_seek_expand_planes), then K7 per plane on that view, set up as ghf_decode_range sets it up (the range begins on a
    // block, so there is no head).
    const uint64_t gA = from / kBlockSymbols, gB = blocks_for(end), nb = gB - gA;
    const size_t segs_per_block = kBlockSymbols / kSegSymbols;
    if (!(rc = grow(c, c->range_dt, elem_bytes))) rc = grow(c, c->range_chunk, nb * elem_bytes, 1024);
    if (!rc) rc = grow(c, c->range_seg, nb * elem_bytes * segs_per_block, 1024 * 64);
    if (rc) return rc;
    SeekExpandPlanesParams a = {};
    for (uint32_t p = 0; p < elem_bytes; ++p) {
      launch_build_decode_tables(d_codes + p, c->range_dt.p + p, c->d_status, c->stream);
      SeekExpandParams& x = a.plane[p];
      x.records = h_table_ptrs[p] + kSeekHeaderBytes;
      x.stream = h_stream_ptrs[p];
      x.stream_bytes = h_stream_bytes[p];
      x.dt = c->range_dt.p + p;
      x.n_symbols = n_elems;
      x.n_blocks = h_infos[p].n_blocks;
      x.g0 = gA;
      x.g1 = gB;
      x.chunk_bit = c->range_chunk.p + p * nb;
      x.seg_bit = c->range_seg.p + p * nb * segs_per_block;
      x.status = c->d_status;
    }
    launch_seek_expand_planes(a, elem_bytes, c->stream);
    for (uint32_t p = 0; p < elem_bytes; ++p) {
      DecParams d = {};
      d.stream = h_stream_ptrs[p];
      d.stream_bytes = h_stream_bytes[p];
      d.dt = c->range_dt.p + p;
      d.chunk_bit = a.plane[p].chunk_bit;
      d.seg_bit = a.plane[p].seg_bit;
      d.n_symbols = end - from;
      d.n_segs = segs_for(d.n_symbols);
      d.no_end_mark = (end == n_elems && !(h_infos[p].flags & GHF_INDEX_NO_END_MARK)) ? 0u : 1u;
      d.out = c->planes.p + p * stride;
      d.out_bytes = nullptr;
      d.status = c->d_status;
      launch_decode(d, c->stream);
    }
  }
  launch_planes_merge_range(c->planes.p, stride, base.p, lead, count, elem_bytes, d_out, c->d_status, c->stream);  // nothing behind a failed decode
  GHF_HIP(c, hipGetLastError());
  return GHF_OK;
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

// ---------------------------------------------------------------------------------------------- zero-suppressed byte planes
// (no reference counterpart)
size_t ghf_sparse_mask_bytes(size_t n) { return n / 8 + (n % 8 != 0); }

int ghf_sparse_split(ghf_ctx* c, const uint8_t* d_in, size_t n, uint8_t* d_mask, uint8_t* d_vals, size_t vals_cap, uint64_t* d_n_vals) {
  if (!c || !d_in || !d_mask || !d_n_vals || (vals_cap && !d_vals)) return GHF_E_INVAL;
  if (!aligned16(d_in) || !aligned16(d_mask) || !aligned16(d_vals) || (reinterpret_cast<uintptr_t>(d_n_vals) & 7u))
    return fail(c, GHF_E_INVAL, "ghf_sparse_split: d_in, d_mask and d_vals must be 16-byte aligned, d_n_vals 8-byte aligned");
  if (n > (size_t)-1 - kSparseTile) return fail(c, GHF_E_INVAL, "ghf_sparse_split: n overflows");
  if (n == 0) return fail(c, GHF_E_EMPTY, "ghf_sparse_split: no bytes");
  GHF_HIP(c, hipSetDevice(c->device));
  launch_sparse_split(d_in, n, d_mask, d_vals, vals_cap, d_n_vals, c->d_sparse_counts, c->d_sparse_offs, c->d_status, c->stream);
  GHF_HIP(c, hipGetLastError());
  return GHF_OK;
}

int ghf_sparse_merge(ghf_ctx* c, const uint8_t* d_mask, const uint8_t* d_vals, size_t n_vals, size_t n, uint8_t* d_out) {
  if (!c || !d_mask || !d_out || (n_vals && !d_vals)) return GHF_E_INVAL;
  if (!aligned16(d_mask) || !aligned16(d_vals) || !aligned16(d_out))
    return fail(c, GHF_E_INVAL, "ghf_sparse_merge: d_mask, d_vals and d_out must be 16-byte aligned");
  if (n > (size_t)-1 - kSparseTile) return fail(c, GHF_E_INVAL, "ghf_sparse_merge: n overflows");
  if (n == 0) return fail(c, GHF_E_EMPTY, "ghf_sparse_merge: no bytes");
  GHF_HIP(c, hipSetDevice(c->device));
  launch_sparse_merge(d_mask, d_vals, n_vals, n, d_out, c->d_sparse_counts, c->d_sparse_offs, c->d_status, c->stream);
  GHF_HIP(c, hipGetLastError());
  return GHF_OK;
}

// sparse_planes as the compress call (GHF_SPARSE_AUTO alone, or bits below elem_bytes) or the decode (bits only) takes it
static inline bool sparse_planes_ok(unsigned sparse_planes, uint32_t elem_bytes, bool may_be_auto) {
  if (sparse_planes == GHF_SPARSE_AUTO) return may_be_auto;
  return (sparse_planes >> elem_bytes) == 0;
}

// raw_planes beside sparse_planes: GHF_RAW_AUTO alone where the call may choose, or bits below
// elem_bytes; a plane has one form, so where both masks are explicit they share no bit
static inline bool forms_ok(unsigned raw_planes, unsigned sparse_planes, uint32_t elem_bytes, bool may_be_auto) {
  if (raw_planes == GHF_RAW_AUTO) return may_be_auto;
  if ((raw_planes >> elem_bytes) != 0) return false;
  return sparse_planes == GHF_SPARSE_AUTO || (raw_planes & sparse_planes) == 0;
}

// the context's second workspace for one sparse plane of n_elems bytes: the mask at [0, *mask_stride), the values behind it
static int sparse_workspace(ghf_ctx* c, size_t n_elems, size_t* mask_stride) {
  *mask_stride = (ghf_sparse_mask_bytes(n_elems) + 255) & ~(size_t)255;
  return grow(c, c->sparse, *mask_stride + ((n_elems + 255) & ~(size_t)255));
}

static void free_indexes(ghf_ctx* c, ghf_index* ix, uint32_t count) {
  for (uint32_t j = 0; j < count; ++j)
    if (ix[j].d_chunk_bit || ix[j].d_seg_bit) (void)free_index_arrays(c, &ix[j]);
  std::memset(ix, 0, count * sizeof *ix);
}

// where the ranked compress calls want the rank tables of their sparse planes; the plain calls want none
struct RankOut {
  bool wanted;
  uint8_t* p;
  size_t slot_bytes;
  bool null() const { return wanted && !p; }
  bool misaligned() const { return wanted && (!aligned16(p) || (slot_bytes & 15u)); }
};
static inline RankOut no_ranks() { return {false, nullptr, 0}; }

static int compress_planes_sparse(ghf_ctx* c, const char* who, const uint8_t* d_in, Base base, size_t n_elems, uint32_t elem_bytes,
                                  unsigned sparse_planes, uint8_t* d_out, size_t slot_bytes, uint64_t* d_out_bytes, ghf_code* d_codes,
                                  ghf_index* h_indexes, unsigned* h_sparse_planes, size_t* h_n_vals, RankOut ranks) {
  if (!c || !d_in || !d_out || !d_out_bytes || !h_sparse_planes || !h_n_vals || base.null() || ranks.null()) return GHF_E_INVAL;
  const std::string f = std::string(who) + ": ";
  if (!elem_bytes_ok(elem_bytes)) return fail(c, GHF_E_INVAL, (f + "elem_bytes must be 2, 4 or 8").c_str());
  if (!aligned16(d_in) || !aligned16(d_out) || (slot_bytes & 15u) || !aligned16(d_codes) || base.misaligned())
    return fail(c, GHF_E_INVAL, (f + "d_in, d_base, d_out, d_codes and slot_bytes must be multiples of 16").c_str());
  if (ranks.misaligned()) return fail(c, GHF_E_INVAL, (f + "d_ranks and rank_slot_bytes must be multiples of 16").c_str());
  if (!sparse_planes_ok(sparse_planes, elem_bytes, true))
    return fail(c, GHF_E_INVAL, (f + "sparse_planes is GHF_SPARSE_AUTO alone or has bits below elem_bytes only").c_str());
  if (workspace_overflow(n_elems, elem_bytes)) return fail(c, GHF_E_INVAL, (f + "n_elems * elem_bytes overflows").c_str());
  if (n_elems == 0) return fail(c, GHF_E_EMPTY, (f + "no elements").c_str());
  if (slot_bytes < ghf_planes_slot_bytes(n_elems)) return fail(c, GHF_E_CAP, (f + "slot_bytes below ghf_planes_slot_bytes(n_elems)").c_str());
  if (ranks.wanted && ranks.slot_bytes < ghf_sparse_rank_bytes(n_elems))
    return fail(c, GHF_E_CAP, (f + "rank_slot_bytes below ghf_sparse_rank_bytes(n_elems)").c_str());
  GHF_HIP(c, hipSetDevice(c->device));
  const uint32_t E = elem_bytes;
  size_t stride = 0, mask_stride = 0;
  int rc = planes_workspace(c, n_elems, E, &stride);
  if (!rc) rc = sparse_workspace(c, n_elems, &mask_stride);
  if (!rc && !d_codes) rc = grow(c, c->batch_codes, 2 * GHF_PLANES_MAX);
  if (rc) return rc;
  ghf_code* codes = d_codes ? d_codes : c->batch_codes.p;
  // compressor.h:63 for all planes in one pass, and THE ONE WAIT of the call: count_p[0] says how many values plane p has
  if ((rc = histogram_planes_into(c, (f + "histogram launch").c_str(), d_in, base.p, n_elems, E, 0, c->d_planes_hists))) return rc;
  uint64_t counts[GHF_PLANES_MAX * GHF_NSYM];
  GHF_HIP(c, hipMemcpyAsync(counts, c->d_planes_hists, (size_t)E * GHF_NSYM * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  GHF_HIP(c, hipStreamSynchronize(c->stream));
  unsigned chosen = 0;
  for (uint32_t p = 0; p < E; ++p) {
    const uint64_t zeros = counts[(size_t)p * GHF_NSYM];
    if (zeros > n_elems) return fail(c, GHF_E_HIP, (f + "the plane counts did not arrive").c_str());
    h_n_vals[p] = n_elems - (size_t)zeros;
    if (sparse_planes == GHF_SPARSE_AUTO ? zeros >= n_elems - n_elems / 4 : (sparse_planes >> p) & 1u) chosen |= 1u << p;
  }
  *h_sparse_planes = chosen;
  const size_t mask_bytes = ghf_sparse_mask_bytes(n_elems);
  if (h_indexes) {  // one side-car per stored stream, of that stream's own symbol count
    std::memset(h_indexes, 0, 2 * E * sizeof *h_indexes);
    for (uint32_t p = 0; p < E && !rc; ++p) {
      const bool sparse = (chosen >> p) & 1u;
      rc = ghf_index_alloc(c, sparse ? mask_bytes : n_elems, &h_indexes[p]);
      if (!rc && sparse && h_n_vals[p]) rc = ghf_index_alloc(c, h_n_vals[p], &h_indexes[E + p]);
    }
    if (rc) {
      free_indexes(c, h_indexes, 2 * E);
      return rc;
    }
  }
  GHF_HIP(c, hipMemsetAsync(d_out_bytes, 0, 2 * E * sizeof(uint64_t), c->stream));  // the empty slots
  launch_planes_split(d_in, base.p, n_elems, E, c->planes.p, stride, c->stream);
  GHF_HIP(c, hipGetLastError());
  uint8_t *d_mask = c->sparse.p, *d_vals = c->sparse.p + mask_stride;
  for (uint32_t p = 0; p < E && !rc; ++p) {
    const uint8_t* plane = c->planes.p + p * stride;
    // K1 has not seen what stands at these addresses now: the workspaces are refilled for every plane
    c->hist.forget();
    c->plan.forget();
    if (!((chosen >> p) & 1u)) {  // what ghf_compress_planes_coded(GHF_PLANES_BUILD_CODES) queues for the plane
      if ((rc = ghf_build_codes(c, c->d_planes_hists + (size_t)p * GHF_NSYM, 1, codes + p, 0))) break;
      if ((rc = ghf_encode_plan(c, plane, n_elems, codes + p, &c->d->total_bits))) break;
      if ((rc = ghf_encode_emit(c, plane, n_elems, codes + p, nullptr, GHF_EMIT_LAST | GHF_EMIT_HEADER, d_out + p * slot_bytes, slot_bytes,
                                h_indexes ? h_indexes + p : nullptr, c->d->end)))
        break;
      launch_store_u64(d_out_bytes + p, &c->d->end[1], 0, c->stream);
      GHF_HIP(c, hipGetLastError());
      continue;
    }
    launch_sparse_split(plane, n_elems, d_mask, d_vals, n_elems, c->d_sparse_offs + kSparseOffWords - 1, c->d_sparse_counts, c->d_sparse_offs,
                        c->d_status, c->stream);
    // the plane's rank table, while its mask stands in the workspace; the split is done with the counts and offsets
    if (ranks.wanted)
      launch_sparse_rank_pack(d_mask, n_elems, ranks.p + p * ranks.slot_bytes, c->d_sparse_counts, c->d_sparse_offs, c->d_status, c->stream);
    GHF_HIP(c, hipGetLastError());
    // compressor.h:62-73 for the mask and for the values, each a byte string of its own
    if ((rc = ghf_compress(c, d_mask, mask_bytes, d_out + p * slot_bytes, slot_bytes, d_out_bytes + p, codes + p,
                           h_indexes ? h_indexes + p : nullptr)))
      break;
    if (h_n_vals[p])
      rc = ghf_compress(c, d_vals, h_n_vals[p], d_out + (E + p) * slot_bytes, slot_bytes, d_out_bytes + E + p, codes + E + p,
                        h_indexes ? h_indexes + E + p : nullptr);
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

// ghf_decode of one stored stream of `symbols` bytes into the workspace at d_to[0 .. cap)
static int decode_stored(ghf_ctx* c, const std::string& f, const uint8_t* d_stream, size_t stream_bytes, const ghf_code* d_code,
                         const ghf_index* index, size_t symbols, uint8_t* d_to, size_t cap) {
  int rc;
  if (!index) {  // the side-car-less path: synchronises, and keeps the side-car for the decode that follows
    uint64_t got = 0;
    if ((rc = ghf_decoded_size(c, d_stream, stream_bytes, d_code, &got))) return rc;
    if (got != symbols) return fail(c, GHF_E_CORRUPT, (f + "a stream does not decode to the size its plane gives it").c_str());
  }
  return ghf_decode(c, d_stream, stream_bytes, d_code, index, d_to, cap, nullptr);
}

static int decode_planes_sparse(ghf_ctx* c, const char* who, const uint8_t* const* h_stream_ptrs, const size_t* h_stream_bytes,
                                const ghf_code* d_codes, const ghf_index* indexes, Base base, unsigned raw_planes, unsigned sparse_planes,
                                const size_t* h_n_vals, size_t n_elems, uint32_t elem_bytes, uint8_t* d_out, size_t cap,
                                uint64_t* d_out_bytes) {
  // the codes of raw planes are not looked at: a tensor of nothing but raw planes needs none
  const bool all_raw = elem_bytes_ok(elem_bytes) && raw_planes == (1u << elem_bytes) - 1u;
  if (!c || !h_stream_ptrs || !h_stream_bytes || (!d_codes && !all_raw) || !d_out || !h_n_vals || base.null()) return GHF_E_INVAL;
  const std::string f = std::string(who) + ": ";
  if (!elem_bytes_ok(elem_bytes)) return fail(c, GHF_E_INVAL, (f + "elem_bytes must be 2, 4 or 8").c_str());
  const uint32_t E = elem_bytes;
  if (!sparse_planes_ok(sparse_planes, E, false))
    return fail(c, GHF_E_INVAL, (f + "sparse_planes has bits below elem_bytes only (the mask the compress call reported)").c_str());
  if (!forms_ok(raw_planes, sparse_planes, E, false))
    return fail(c, GHF_E_INVAL, (f + "raw_planes has bits below elem_bytes only, none of them a sparse plane's").c_str());
  const size_t mask_bytes = ghf_sparse_mask_bytes(n_elems);
  auto raw = [&](uint32_t p) { return ((raw_planes >> p) & 1u) != 0; };
  // slot j is stored when it is a plane's own slot, or the values slot of a sparse plane that has values
  auto symbols_of = [&](uint32_t j) -> size_t {
    const uint32_t p = j % E;
    const bool sparse = (sparse_planes >> p) & 1u;
    if (j < E) return sparse ? mask_bytes : n_elems;
    return sparse ? h_n_vals[p] : 0;
  };
  for (uint32_t p = 0; p < E; ++p)
    if (((sparse_planes >> p) & 1u) && h_n_vals[p] > n_elems) return fail(c, GHF_E_INVAL, (f + "a plane has more values than elements").c_str());
  for (uint32_t j = 0; j < 2 * E; ++j)
    if ((j < E || symbols_of(j)) && (!h_stream_ptrs[j] || !aligned16(h_stream_ptrs[j])))
      return fail(c, GHF_E_INVAL, (f + "a stream pointer is null or not 16-byte aligned").c_str());
  if (!aligned16(d_out) || base.misaligned()) return fail(c, GHF_E_INVAL, (f + "d_out and d_base must be 16-byte aligned").c_str());
  if (workspace_overflow(n_elems, E)) return fail(c, GHF_E_INVAL, (f + "n_elems * elem_bytes overflows").c_str());
  for (uint32_t j = 0; indexes && j < 2 * E; ++j)
    if ((j < E || symbols_of(j)) && !raw(j % E) && (indexes[j].n_symbols != symbols_of(j) || !index_is_whole(&indexes[j])))
      return fail(c, GHF_E_INVAL, (f + "an index does not cover exactly the symbols of its stream").c_str());
  for (uint32_t p = 0; p < E; ++p)  // a raw plane is its n_elems bytes and nothing else
    if (raw(p) && h_stream_bytes[p] != n_elems) return fail(c, GHF_E_INVAL, (f + "a raw plane does not have n_elems bytes").c_str());
  if (n_elems == 0) return fail(c, GHF_E_EMPTY, (f + "no elements").c_str());
  if (cap < n_elems * E) return fail(c, GHF_E_CAP, (f + "output capacity below n_elems * elem_bytes").c_str());
  GHF_HIP(c, hipSetDevice(c->device));
  size_t stride = 0, mask_stride = 0;
  int rc = all_raw ? GHF_OK : planes_workspace(c, n_elems, E, &stride);
  if (!rc && sparse_planes) rc = sparse_workspace(c, n_elems, &mask_stride);
  if (rc) return rc;
  for (uint32_t p = 0; p < E; ++p) {
    if (raw(p)) continue;  // never copied: the merge reads it where it lies
    uint8_t* plane = c->planes.p + p * stride;
    if (!((sparse_planes >> p) & 1u)) {
      if ((rc = decode_stored(c, f, h_stream_ptrs[p], h_stream_bytes[p], d_codes + p, indexes ? indexes + p : nullptr, n_elems, plane, stride)))
        return rc;
      continue;
    }
    uint8_t *d_mask = c->sparse.p, *d_vals = c->sparse.p + mask_stride;
    if ((rc = decode_stored(c, f, h_stream_ptrs[p], h_stream_bytes[p], d_codes + p, indexes ? indexes + p : nullptr, mask_bytes, d_mask,
                            mask_stride)))
      return rc;
    if (h_n_vals[p] &&
        (rc = decode_stored(c, f, h_stream_ptrs[E + p], h_stream_bytes[E + p], d_codes + E + p, indexes ? indexes + E + p : nullptr,
                            h_n_vals[p], d_vals, c->sparse.cap - mask_stride)))
      return rc;
    launch_sparse_merge(d_mask, d_vals, h_n_vals[p], n_elems, plane, c->d_sparse_counts, c->d_sparse_offs, c->d_status, c->stream);
    GHF_HIP(c, hipGetLastError());
  }
  // nothing is stored behind a latched status
  if (!raw_planes) {
    launch_planes_merge(c->planes.p, stride, base.p, n_elems, E, d_out, c->d_status, c->stream);
  } else {
    const uint8_t* from[GHF_PLANES_MAX];
    for (uint32_t p = 0; p < E; ++p) from[p] = raw(p) ? h_stream_ptrs[p] : c->planes.p + p * stride;
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
static inline uint64_t rank_blocks_for(uint64_t n) { return n / kSparseRankElems + (n % kSparseRankElems != 0); }

size_t ghf_sparse_rank_bytes(size_t n) { return kSparseRankHeaderBytes + 8 * ((size_t)rank_blocks_for(n) + 1); }

int ghf_sparse_rank_pack(ghf_ctx* c, const uint8_t* d_mask, size_t n, uint8_t* d_table, size_t cap) {
  if (!c || !d_mask || !d_table) return GHF_E_INVAL;
  if (!aligned16(d_mask) || !aligned16(d_table)) return fail(c, GHF_E_INVAL, "ghf_sparse_rank_pack: d_mask and d_table must be 16-byte aligned");
  if (n > (size_t)-1 - kSparseRankElems) return fail(c, GHF_E_INVAL, "ghf_sparse_rank_pack: n overflows");
  if (n == 0) return fail(c, GHF_E_EMPTY, "ghf_sparse_rank_pack: no bytes");
  if (cap < ghf_sparse_rank_bytes(n)) return fail(c, GHF_E_CAP, "ghf_sparse_rank_pack: table capacity below ghf_sparse_rank_bytes(n)");
  GHF_HIP(c, hipSetDevice(c->device));
  launch_sparse_rank_pack(d_mask, n, d_table, c->d_sparse_counts, c->d_sparse_offs, c->d_status, c->stream);
  GHF_HIP(c, hipGetLastError());
  return GHF_OK;
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
  GHF_HIP(c, hipSetDevice(c->device));
  launch_sparse_merge_at(d_mask, d_vals, vals_skip, n_vals, n, d_out, c->d_sparse_counts, c->d_sparse_offs, c->d_status, c->stream);
  GHF_HIP(c, hipGetLastError());
  return GHF_OK;
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

// one stored stream of a range call: which symbols of it the call decodes, and where to
struct RangePart {
  uint32_t slot;      // in the caller's arrays of 2 * elem_bytes
  uint64_t lo, hi;    // symbols [lo, hi) of the stream; lo is a multiple of kBlockSymbols
  uint64_t symbols;   // of the whole stream
  uint8_t* to;        // symbol lo lands here (16-byte aligned)
  size_t cap;
};

static int decode_planes_sparse_range(ghf_ctx* c, const char* who, const uint8_t* const* h_stream_ptrs, const size_t* h_stream_bytes,
                                      const ghf_code* d_codes, const ghf_index* indexes, const ghf_seek_info* h_infos,
                                      const uint8_t* const* h_table_ptrs, const size_t* h_table_bytes,
                                      const ghf_sparse_rank_info* h_rank_infos, const uint8_t* const* h_rank_ptrs, Base base,
                                      unsigned raw_planes, unsigned sparse_planes, size_t n_elems, uint32_t elem_bytes, uint64_t first,
                                      uint64_t count, uint8_t* d_out, size_t cap) {
  // the codes of raw planes are not looked at: a tensor of nothing but raw planes needs none
  const bool all_raw = elem_bytes_ok(elem_bytes) && raw_planes == (1u << elem_bytes) - 1u;
  if (!c || !h_stream_ptrs || !h_stream_bytes || (!d_codes && !all_raw) || !d_out || base.null()) return GHF_E_INVAL;
  const std::string f = std::string(who) + ": ";
  if (!elem_bytes_ok(elem_bytes)) return fail(c, GHF_E_INVAL, (f + "elem_bytes must be 2, 4 or 8").c_str());
  const uint32_t E = elem_bytes;
  const bool by_table = h_infos || h_table_ptrs || h_table_bytes;
  if ((indexes != nullptr) == by_table || (by_table && !(h_infos && h_table_ptrs && h_table_bytes)))
    return fail(c, GHF_E_INVAL, (f + "exactly one of indexes / (h_infos, h_table_ptrs, h_table_bytes) must be given").c_str());
  // a raw plane has a stream pointer and a size and nothing else: its index, info and table are not read
  auto raw = [&](uint32_t p) { return ((raw_planes >> p) & 1u) != 0; };
  // what ghf_decode_planes_range asks of a plane, of one stored stream
  auto pointers_ok = [&](uint32_t j) {
    return h_stream_ptrs[j] && aligned16(h_stream_ptrs[j]) && (!by_table || raw(j) || (h_table_ptrs[j] && aligned16(h_table_ptrs[j])));
  };
  auto symbols_of = [&](uint32_t j) -> uint64_t { return by_table ? h_infos[j].n_symbols : indexes[j].n_symbols; };
  auto index_ok = [&](uint32_t j) { return by_table || indexes[j].n_symbols == 0 || index_is_whole(&indexes[j]); };
  for (uint32_t p = 0; p < E; ++p)
    if (!pointers_ok(p)) return fail(c, GHF_E_INVAL, (f + "a stream or table pointer is null or not 16-byte aligned").c_str());
  if (!aligned16(d_out) || base.misaligned()) return fail(c, GHF_E_INVAL, (f + "d_out and d_base must be 16-byte aligned").c_str());
  for (uint32_t p = 0; p < E; ++p)
    if (!raw(p) && !index_ok(p)) return fail(c, GHF_E_INVAL, (f + "malformed index").c_str());
  if (first > n_elems || count > n_elems - first) return fail(c, GHF_E_INVAL, (f + "first + count exceeds n_elems").c_str());
  // the workspace holds the range from the start of its first rank block to the end of its last, and a vector more
  const size_t slack = 2 * (size_t)kSparseRankElems + 16;
  if (count > (size_t)-1 - slack || workspace_overflow((size_t)count + slack, E))
    return fail(c, GHF_E_INVAL, (f + "count * elem_bytes overflows").c_str());
  for (uint32_t p = 0; by_table && p < E; ++p) {
    if (raw(p)) continue;
    const int rc = seek_table_ok(c, who, h_infos + p, h_table_ptrs[p], h_table_bytes[p]);
    if (rc) return rc;
  }
  if (cap < count * E) return fail(c, GHF_E_CAP, (f + "output capacity below count * elem_bytes").c_str());
  // ... and what the sparse form adds
  if (!sparse_planes_ok(sparse_planes, E, false))
    return fail(c, GHF_E_INVAL, (f + "sparse_planes has bits below elem_bytes only (the mask the compress call reported)").c_str());
  // ... and the raw form
  if (!forms_ok(raw_planes, sparse_planes, E, false))
    return fail(c, GHF_E_INVAL, (f + "raw_planes has bits below elem_bytes only, none of them a sparse plane's").c_str());
  for (uint32_t p = 0; p < E; ++p)
    if (raw(p) && h_stream_bytes[p] != n_elems) return fail(c, GHF_E_INVAL, (f + "a raw plane does not have n_elems bytes").c_str());
  if (sparse_planes && (!h_rank_infos || !h_rank_ptrs)) return fail(c, GHF_E_INVAL, (f + "sparse planes need their rank tables").c_str());
  const uint64_t mask_bytes = ghf_sparse_mask_bytes(n_elems);
  for (uint32_t p = 0; p < E; ++p) {
    if (!((sparse_planes >> p) & 1u)) continue;
    if (!h_rank_ptrs[p]) return fail(c, GHF_E_INVAL, (f + "a sparse plane has no rank table").c_str());
    if (h_rank_infos[p].n != n_elems) return fail(c, GHF_E_INVAL, (f + "a rank table is not one of n_elems elements").c_str());
    if (h_rank_infos[p].version != kSparseRankVersion || h_rank_infos[p].n_blocks != rank_blocks_for(n_elems) || h_rank_infos[p].n_vals > n_elems)
      return fail(c, GHF_E_FORMAT, (f + "a rank info is not what ghf_sparse_rank_parse fills in").c_str());
  }
  for (uint32_t p = 0; p < E; ++p) {
    if (raw(p)) continue;
    const bool sparse = (sparse_planes >> p) & 1u;
    if (symbols_of(p) != (sparse ? mask_bytes : (uint64_t)n_elems))
      return fail(c, GHF_E_INVAL, sparse ? (f + "a mask stream does not have ghf_sparse_mask_bytes(n_elems) symbols").c_str()
                                         : (f + "a dense stream does not have n_elems symbols").c_str());
    if (!sparse || h_rank_infos[p].n_vals == 0) continue;  // the values slot of any other plane is ignored
    if (!pointers_ok(E + p)) return fail(c, GHF_E_INVAL, (f + "a stream or table pointer is null or not 16-byte aligned").c_str());
    if (!index_ok(E + p)) return fail(c, GHF_E_INVAL, (f + "malformed index").c_str());
    if (symbols_of(E + p) != h_rank_infos[p].n_vals)
      return fail(c, GHF_E_INVAL, (f + "a values stream does not have the symbols its rank table counts").c_str());
    if (by_table) {
      const int rc = seek_table_ok(c, who, h_infos + E + p, h_table_ptrs[E + p], h_table_bytes[E + p]);
      if (rc) return rc;
    }
  }
  if (count == 0) return GHF_OK;
  if (!sparse_planes && !raw_planes)  // nothing sparse: the origin of section 17, and its call
    return decode_planes_range(c, who, h_stream_ptrs, h_stream_bytes, d_codes, indexes, h_infos, h_table_ptrs, h_table_bytes, base, E, first,
                               count, d_out, cap);
  // THE PLAN.  The common origin of all planes is the start of the rank block that holds `first`: a multiple of 4096 for a
  // dense plane, of 4096 mask bytes for a mask, and the values in front of it number cum[b0].  A sparse plane is rebuilt for the
  // whole rank blocks [b0, b1) (cut at n_elems): the sub-string's mask bytes are whole, so its last mask byte obeys the pad rule.
  // With raw planes and no sparse one the origin is section 17's, the start of the seek block that holds `first`.  A raw plane has
  // no part in the plan: nothing of it is decoded or copied, the merge reads it at stream + first.
  const uint64_t origin = sparse_planes ? kSparseRankElems : kBlockSymbols;
  const uint64_t from = first - first % origin, end = first + count;
  const uint64_t b0 = from / kSparseRankElems, b1 = rank_blocks_for(end);
  const uint64_t sub_n = (sparse_planes ? std::min<uint64_t>(b1 * kSparseRankElems, n_elems) : end) - from;
  const uint64_t m_lo = b0 * (kSparseRankElems / 8), m_hi = std::min<uint64_t>(b1 * (kSparseRankElems / 8), mask_bytes);
  uint64_t v_lo[GHF_PLANES_MAX] = {}, v_hi[GHF_PLANES_MAX] = {};
  for (uint32_t p = 0; p < E; ++p) {
    if (!((sparse_planes >> p) & 1u)) continue;
    const uint8_t* cum = h_rank_ptrs[p] + kSparseRankHeaderBytes;
    v_lo[p] = le64(cum + 8 * b0);
    v_hi[p] = le64(cum + 8 * b1);
    if (v_lo[p] > v_hi[p] || v_hi[p] > h_rank_infos[p].n_vals || v_hi[p] - v_lo[p] > sub_n)
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
    if (raw(p)) continue;
    if (!((sparse_planes >> p) & 1u)) {
      parts[n_parts++] = {p, from, end, n_elems, c->planes.p + p * stride, stride};
      continue;
    }
    parts[n_parts++] = {p, m_lo, m_hi, mask_bytes, d_mask, mask_stride};
    if (v_hi[p] > v_lo[p]) parts[n_parts++] = {E + p, v_lo[p] - v_lo[p] % kBlockSymbols, v_hi[p], h_rank_infos[p].n_vals, d_vals, vals_room};
  }
  // behind the last stored stream of a sparse plane (its values, or its mask when the sub-string has none): the plane's merge
  auto merge_behind = [&](uint32_t j) {
    const uint32_t p = j % E;
    if (((sparse_planes >> p) & 1u) && (j >= E || v_hi[p] == v_lo[p]))
      launch_sparse_merge_at(d_mask, d_vals, v_lo[p] % kBlockSymbols, v_hi[p] - v_lo[p], sub_n, c->planes.p + p * stride, c->d_sparse_counts,
                             c->d_sparse_offs, c->d_status, c->stream);
  };
  if (!n_parts) {
    // every plane is raw: the merge below is the whole call
  } else if (by_table) {
    // One launch expands the covered blocks of every stored stream (k_seek_expand_streams): expanding each by itself would
    // pay k_seek_expand's latency floor up to 2 E times (DESIGN.md section 17 has the measurement).  Every stream gets tables of
    // its own, alive until its K7 has run.
    const size_t segs_per_block = kBlockSymbols / kSegSymbols;
    size_t blocks = 0;
    for (uint32_t i = 0; i < n_parts; ++i) blocks += (size_t)(blocks_for(parts[i].hi) - parts[i].lo / kBlockSymbols);
    if (!(rc = grow(c, c->range_dt, 2 * GHF_PLANES_MAX))) rc = grow(c, c->range_chunk, blocks, 1024);
    if (!rc) rc = grow(c, c->range_seg, blocks * segs_per_block, 1024 * 64);
    if (rc) return rc;
    SeekExpandStreamsParams a = {};
    size_t at = 0;
    uint32_t stored = 0;
    for (uint32_t i = 0; i < n_parts; ++i) stored |= 1u << parts[i].slot;
    launch_build_decode_tables_slots(d_codes, c->range_dt.p, 2 * E, stored, c->d_status, c->stream);  // range_dt[j]: the tables of slot j
    for (uint32_t i = 0; i < n_parts; ++i) {
      const uint32_t j = parts[i].slot;
      SeekExpandParams& x = a.stream[i];
      x.records = h_table_ptrs[j] + kSeekHeaderBytes;
      x.stream = h_stream_ptrs[j];
      x.stream_bytes = h_stream_bytes[j];
      x.dt = c->range_dt.p + j;
      x.n_symbols = parts[i].symbols;
      x.n_blocks = h_infos[j].n_blocks;
      x.g0 = parts[i].lo / kBlockSymbols;
      x.g1 = blocks_for(parts[i].hi);
      x.chunk_bit = c->range_chunk.p + at;
      x.seg_bit = c->range_seg.p + at * segs_per_block;
      x.status = c->d_status;
      at += (size_t)(x.g1 - x.g0);
    }
    launch_seek_expand_streams(a, n_parts, c->stream);
    GHF_HIP(c, hipGetLastError());
    for (uint32_t i = 0; i < n_parts; ++i) {  // K7 on the expanded view, set up as ghf_decode_planes_range sets it up
      const uint32_t j = parts[i].slot;
      DecParams d = {};
      d.stream = h_stream_ptrs[j];
      d.stream_bytes = h_stream_bytes[j];
      d.dt = c->range_dt.p + j;
      d.chunk_bit = a.stream[i].chunk_bit;
      d.seg_bit = a.stream[i].seg_bit;
      d.n_symbols = parts[i].hi - parts[i].lo;
      d.n_segs = segs_for(d.n_symbols);
      d.no_end_mark = (parts[i].hi == parts[i].symbols && !(h_infos[j].flags & GHF_INDEX_NO_END_MARK)) ? 0u : 1u;
      d.out = parts[i].to;
      d.out_bytes = nullptr;
      d.status = c->d_status;
      launch_decode(d, c->stream);
      merge_behind(j);
    }
  } else {
    for (uint32_t i = 0; i < n_parts; ++i) {
      const uint32_t j = parts[i].slot;
      if ((rc = ghf_decode_range(c, h_stream_ptrs[j], h_stream_bytes[j], d_codes + j, indexes + j, nullptr, nullptr, 0, parts[i].lo,
                                 parts[i].hi - parts[i].lo, parts[i].to, parts[i].cap)))
        return rc;
      merge_behind(j);
    }
  }
  // nothing reaches d_out behind a failed decode or a count that does not match the rank table
  if (!raw_planes) {
    launch_planes_merge_range(c->planes.p, stride, base.p, first - from, count, E, d_out, c->d_status, c->stream);
  } else {
    // the workspace planes start 256-byte aligned at element `from`, a multiple of 4096, and a raw plane 16-byte aligned at
    // element 0: the run's first byte stands first % 16 behind a vector in every one of them
    const uint8_t* src[GHF_PLANES_MAX];
    for (uint32_t p = 0; p < E; ++p) src[p] = raw(p) ? h_stream_ptrs[p] + first : c->planes.p + p * stride + (first - from);
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
// (no reference counterpart).  In this family d_base is optional: null is the plain call
static inline Base base_opt(const uint8_t* d_base) { return d_base ? base_of(d_base) : no_base(); }

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
  GHF_HIP(c, hipSetDevice(c->device));
  launch_planes_split_to(d_in, d_base, n_elems, elem_bytes, h_plane_ptrs, c->stream);
  GHF_HIP(c, hipGetLastError());
  return GHF_OK;
}

int ghf_planes_merge_from(ghf_ctx* c, const uint8_t* const* h_plane_ptrs, const uint8_t* d_base, size_t n_elems, uint32_t elem_bytes,
                          uint8_t* d_out) {
  uint32_t skew = 0;
  const int rc = plane_ptrs_args(c, "ghf_planes_merge_from", d_out, h_plane_ptrs, d_base, n_elems, elem_bytes, &skew);
  if (rc) return rc;
  if (skew) return fail(c, GHF_E_INVAL, "ghf_planes_merge_from: the plane pointers must be 16-byte aligned");
  GHF_HIP(c, hipSetDevice(c->device));
  launch_planes_merge_from(h_plane_ptrs, d_base, n_elems, elem_bytes, d_out, nullptr, c->stream);
  GHF_HIP(c, hipGetLastError());
  return GHF_OK;
}

int ghf_planes_merge_range_from(ghf_ctx* c, const uint8_t* const* h_plane_ptrs, const uint8_t* d_base, size_t count, uint32_t elem_bytes,
                                uint8_t* d_out) {
  uint32_t skew = 0;
  const int rc = plane_ptrs_args(c, "ghf_planes_merge_range_from", d_out, h_plane_ptrs, d_base, count, elem_bytes, &skew);
  if (rc) return rc;
  GHF_HIP(c, hipSetDevice(c->device));
  launch_planes_merge_from(h_plane_ptrs, d_base, count, elem_bytes, d_out, nullptr, c->stream);  // the common skew picks the kernel
  GHF_HIP(c, hipGetLastError());
  return GHF_OK;
}

int ghf_compress_planes_forms(ghf_ctx* c, const uint8_t* d_in, const uint8_t* d_base, size_t n_elems, uint32_t elem_bytes,
                              unsigned raw_planes, unsigned sparse_planes, uint8_t* d_out, size_t slot_bytes, uint64_t* d_out_bytes,
                              ghf_code* d_codes, ghf_index* h_indexes, uint8_t* d_ranks, size_t rank_slot_bytes, unsigned* h_raw_planes,
                              unsigned* h_sparse_planes, size_t* h_n_vals) {
  if (!c || !d_in || !d_out || !d_out_bytes || !h_raw_planes || !h_sparse_planes || !h_n_vals) return GHF_E_INVAL;
  const char* f = "ghf_compress_planes_forms: ";
  auto say = [&](const char* what) { return std::string(f) + what; };
  if (!elem_bytes_ok(elem_bytes)) return fail(c, GHF_E_INVAL, say("elem_bytes must be 2, 4 or 8").c_str());
  const uint32_t E = elem_bytes;
  if (!aligned16(d_in) || !aligned16(d_out) || (slot_bytes & 15u) || !aligned16(d_codes) || !aligned16(d_base))
    return fail(c, GHF_E_INVAL, say("d_in, d_base, d_out, d_codes and slot_bytes must be multiples of 16").c_str());
  if (d_ranks && (!aligned16(d_ranks) || (rank_slot_bytes & 15u)))
    return fail(c, GHF_E_INVAL, say("d_ranks and rank_slot_bytes must be multiples of 16").c_str());
  if (!sparse_planes_ok(sparse_planes, E, true))
    return fail(c, GHF_E_INVAL, say("sparse_planes is GHF_SPARSE_AUTO alone or has bits below elem_bytes only").c_str());
  if (!forms_ok(raw_planes, sparse_planes, E, true))
    return fail(c, GHF_E_INVAL, say("raw_planes is GHF_RAW_AUTO alone or has bits below elem_bytes only, none of them a sparse plane's").c_str());
  if (workspace_overflow(n_elems, E)) return fail(c, GHF_E_INVAL, say("n_elems * elem_bytes overflows").c_str());
  if (n_elems == 0) return fail(c, GHF_E_EMPTY, say("no elements").c_str());
  if (slot_bytes < ghf_planes_slot_bytes(n_elems)) return fail(c, GHF_E_CAP, say("slot_bytes below ghf_planes_slot_bytes(n_elems)").c_str());
  if (d_ranks && rank_slot_bytes < ghf_sparse_rank_bytes(n_elems))
    return fail(c, GHF_E_CAP, say("rank_slot_bytes below ghf_sparse_rank_bytes(n_elems)").c_str());
  GHF_HIP(c, hipSetDevice(c->device));
  const bool raw_auto = raw_planes == GHF_RAW_AUTO, sparse_auto = sparse_planes == GHF_SPARSE_AUTO;
  const unsigned all = (1u << E) - 1u;
  // the counts are needed on the HOST for a choice and for the value counts of sparse planes, on the device for every code
  const bool wait = raw_auto || sparse_auto || sparse_planes != 0;
  int rc = GHF_OK;
  // [0, 2 MAX): the codes of the stored streams when the caller wants none; [2 MAX, 3 MAX): the codes the choice is priced with
  if ((rc = grow(c, c->batch_codes, 3 * GHF_PLANES_MAX))) return rc;
  ghf_code* codes = d_codes ? d_codes : c->batch_codes.p;
  ghf_code* priced = c->batch_codes.p + 2 * GHF_PLANES_MAX;
  uint64_t* d_prices = c->d_planes_hists + (size_t)GHF_PLANES_MAX * GHF_NSYM;
  if (wait || raw_planes != all)
    if ((rc = histogram_planes_into(c, say("histogram launch").c_str(), d_in, d_base, n_elems, E, 0, c->d_planes_hists))) return rc;
  unsigned raw_chosen = raw_auto ? 0u : raw_planes, sparse_chosen = sparse_auto ? 0u : sparse_planes;
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
      if (zeros > n_elems) return fail(c, GHF_E_HIP, say("the plane counts did not arrive").c_str());
      h_n_vals[p] = n_elems - (size_t)zeros;
      if (sparse_auto && !((raw_chosen >> p) & 1u) && sparse_pays && zeros >= n_elems - n_elems / 4) sparse_chosen |= 1u << p;
      // prices[p] == 0: the plane has no code (a count at or above 2^55); it stays dense, and the dense path latches why
      if (raw_auto && !((sparse_chosen >> p) & 1u) && prices[p] >= n_elems) raw_chosen |= 1u << p;
    }
  }
  *h_raw_planes = raw_chosen;
  *h_sparse_planes = sparse_chosen;
  auto raw = [&](uint32_t p) { return ((raw_chosen >> p) & 1u) != 0; };
  auto sparse = [&](uint32_t p) { return ((sparse_chosen >> p) & 1u) != 0; };
  size_t stride = 0, mask_stride = 0;
  if (raw_chosen != all) rc = planes_workspace(c, n_elems, E, &stride);
  if (!rc && sparse_chosen) rc = sparse_workspace(c, n_elems, &mask_stride);
  if (rc) return rc;
  const size_t mask_bytes = ghf_sparse_mask_bytes(n_elems);
  if (h_indexes) {  // one side-car per stream that has a code, of that stream's own symbol count; a raw plane has none
    std::memset(h_indexes, 0, 2 * E * sizeof *h_indexes);
    for (uint32_t p = 0; p < E && !rc; ++p) {
      if (raw(p)) continue;
      rc = ghf_index_alloc(c, sparse(p) ? mask_bytes : n_elems, &h_indexes[p]);
      if (!rc && sparse(p) && h_n_vals[p]) rc = ghf_index_alloc(c, h_n_vals[p], &h_indexes[E + p]);
    }
    if (rc) {
      free_indexes(c, h_indexes, 2 * E);
      return rc;
    }
  }
  GHF_HIP(c, hipMemsetAsync(d_out_bytes, 0, 2 * E * sizeof(uint64_t), c->stream));  // the empty slots
  // the split writes a raw plane straight into its slot and every other plane into the workspace
  if (!raw_chosen) {
    launch_planes_split(d_in, d_base, n_elems, E, c->planes.p, stride, c->stream);
  } else {
    uint8_t* to[GHF_PLANES_MAX];
    for (uint32_t p = 0; p < E; ++p) to[p] = raw(p) ? d_out + p * slot_bytes : c->planes.p + p * stride;
    launch_planes_split_to(d_in, d_base, n_elems, E, to, c->stream);
  }
  GHF_HIP(c, hipGetLastError());
  uint8_t *d_mask = c->sparse.p, *d_vals = c->sparse.p + mask_stride;
  for (uint32_t p = 0; p < E && !rc; ++p) {
    if (raw(p)) {
      launch_store_u64(d_out_bytes + p, nullptr, (uint64_t)n_elems, c->stream);
      GHF_HIP(c, hipGetLastError());
      continue;
    }
    const uint8_t* plane = c->planes.p + p * stride;
    // K1 has not seen what stands at these addresses now: the workspaces are refilled for every plane
    c->hist.forget();
    c->plan.forget();
    if (!sparse(p)) {  // what ghf_compress_planes_coded(GHF_PLANES_BUILD_CODES) queues for the plane
      const ghf_code* code = raw_auto ? priced + p : codes + p;
      if (!raw_auto && (rc = ghf_build_codes(c, c->d_planes_hists + (size_t)p * GHF_NSYM, 1, codes + p, 0))) break;
      if ((rc = ghf_encode_plan(c, plane, n_elems, code, &c->d->total_bits))) break;
      if ((rc = ghf_encode_emit(c, plane, n_elems, code, nullptr, GHF_EMIT_LAST | GHF_EMIT_HEADER, d_out + p * slot_bytes, slot_bytes,
                                h_indexes ? h_indexes + p : nullptr, c->d->end)))
        break;
      launch_store_u64(d_out_bytes + p, &c->d->end[1], 0, c->stream);
      GHF_HIP(c, hipGetLastError());
      if (raw_auto && d_codes) GHF_HIP(c, hipMemcpyAsync(d_codes + p, code, sizeof(ghf_code), hipMemcpyDeviceToDevice, c->stream));
      continue;
    }
    launch_sparse_split(plane, n_elems, d_mask, d_vals, n_elems, c->d_sparse_offs + kSparseOffWords - 1, c->d_sparse_counts, c->d_sparse_offs,
                        c->d_status, c->stream);
    // the plane's rank table, while its mask stands in the workspace; the split is done with the counts and offsets
    if (d_ranks) launch_sparse_rank_pack(d_mask, n_elems, d_ranks + p * rank_slot_bytes, c->d_sparse_counts, c->d_sparse_offs, c->d_status, c->stream);
    GHF_HIP(c, hipGetLastError());
    // compressor.h:62-73 for the mask and for the values, each a byte string of its own
    if ((rc = ghf_compress(c, d_mask, mask_bytes, d_out + p * slot_bytes, slot_bytes, d_out_bytes + p, codes + p,
                           h_indexes ? h_indexes + p : nullptr)))
      break;
    if (h_n_vals[p])
      rc = ghf_compress(c, d_vals, h_n_vals[p], d_out + (E + p) * slot_bytes, slot_bytes, d_out_bytes + E + p, codes + E + p,
                        h_indexes ? h_indexes + E + p : nullptr);
  }
  c->hist.forget();
  c->plan.forget();
  return rc;
}

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

}  // extern "C"
