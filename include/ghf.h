/* include/ghf.h -- C ABI of libghf.so: the MI355X (gfx950) canonical-Huffman hot path.
 *
 * Drop-in boundary for the byte-keyed canonical-Huffman path of chenghuige/golden-huffman (`glzip`).
 * Each entry point names the reference interface it replaces (file:line relative to the reference
 * tree).  Plain pointers and sizes only; no C++/torch/HIP types cross this boundary (a HIP stream is
 * passed as void*).  Every pointer whose name starts with d_ is DEVICE memory on the context's GPU
 * and must be 16-byte aligned unless stated otherwise; everything else is host memory.
 *
 * All stage calls are asynchronous on the context's stream and never synchronise with the host.
 * Device-side failures (code longer than 32 bits, empty input, output capacity exceeded) are latched
 * in a device status word; ghf_sync() / ghf_status() return them.  No call throws.
 *
 * The product path has no CPU fallback: without a HIP device every stage call returns GHF_E_HIP.
 */
#ifndef GHF_H_
#define GHF_H_
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GHF_NSYM 257 /* include/type_traits.h:50 CharSymbolNum = 256 byte values + end-of-stream mark */

enum ghf_status_code {
  GHF_OK = 0,
  GHF_E_INVAL = 1,   /* bad argument (null, misaligned, ...) */
  GHF_E_HIP = 2,     /* HIP runtime error / no device; see ghf_last_error() */
  GHF_E_EMPTY = 3,   /* n == 0: the reference is undefined there; we refuse */
  GHF_E_CODELEN = 4, /* a code longer than 32 bits (reference limit, include/canonical_huff_encoder.h:43-44) */
  GHF_E_CAP = 5,     /* output capacity too small */
  GHF_E_FORMAT = 6,  /* not a .crs2 header */
  GHF_E_CORRUPT = 7, /* stream does not decode to the expected symbol count / end mark */
  GHF_E_NOMEM = 8,
  GHF_E_SINGLE = 9, /* .crs only: one distinct byte value -- the lone leaf gets the empty code and the reference's
                       decoder dereferences a NULL child (include/huff_tree.cc:255-271); undefined there, refused here */
  GHF_E_NOCODE = 10 /* shared-code batches: an item holds a byte value to which the shared code gives no code;
                       ghf_compress_planes_coded: a plane holds a byte value to which the caller's d_codes[p] gives none */
};

/* The encoder's tables -- mirrors the private members of CanonicalHuffEncoder,
 * include/canonical_huff_encoder.h:107-120 (length_, codeword_, symbol_, first_code_, start_pos_,
 * min_len_, max_len_).  first_code/start_pos are indexed from 1 like the reference's. */
typedef struct ghf_code {
  uint32_t length[GHF_NSYM];
  uint32_t codeword[GHF_NSYM];
  uint32_t symbol[GHF_NSYM]; /* unused tail = 0xFFFFFFFF (canonical_huff_encoder.cc:88) */
  uint32_t first_code[64];   /* 1024 for len < min_len (canonical_huff_encoder.cc:119-121) */
  uint32_t start_pos[64];
  int32_t min_len;
  int32_t max_len;
} ghf_code;

/* Side-car index for block-parallel decode (no reference counterpart: the .crs2 wire format has no
 * sync points).  It is NOT part of the .crs2 bytes.  The struct lives on the host;
 * the two arrays are device memory (ghf_index_alloc). */
typedef struct ghf_index {
  uint64_t n_symbols;     /* input bytes covered */
  uint32_t chunk_symbols; /* symbols per index block (4096 = 64 segments) */
  uint32_t seg_symbols;   /* symbols per segment (64) */
  uint64_t n_chunks;      /* index blocks */
  uint64_t n_segs;
  uint32_t flags;    /* GHF_INDEX_NO_END_MARK: the buffer is a shard that was emitted without GHF_EMIT_LAST */
  uint32_t reserved;
  uint64_t* d_chunk_bit; /* [n_chunks] bit offset of each block's first code, counted from byte 0 of the d_out the
                            emit call wrote into (= absolute stream bit, header included, unless GHF_EMIT_REBASE) */
  uint32_t* d_seg_bit;   /* [n_segs]   bit offset of each segment's END relative to its block's first code (a segment
                            starts where its predecessor in the block ends; the first one at the block's first code) */
} ghf_index;

#define GHF_INDEX_NO_END_MARK 1u

typedef struct ghf_ctx ghf_ctx;

/* ---- context (the reference has none: single-threaded objects; SURVEY 8b "Threading") ---------- */
int ghf_ctx_create(int device, ghf_ctx** out);
int ghf_ctx_destroy(ghf_ctx* ctx);
/* A new context owns a private non-blocking stream.  ghf_ctx_set_stream makes it queue on the caller's
 * hipStream_t instead (NULL = HIP's default stream), e.g. torch's current stream. */
int ghf_ctx_set_stream(ghf_ctx* ctx, void* hip_stream);
int ghf_sync(ghf_ctx* ctx);                             /* wait for the stream; returns latched device status */
int ghf_status(ghf_ctx* ctx);                           /* = ghf_sync */
int ghf_clear_status(ghf_ctx* ctx);
const char* ghf_last_error(ghf_ctx* ctx);
const char* ghf_status_string(int status);
int ghf_version(void);

/* ---- memory helpers, so that C/C++ hosts need no HIP headers.  They replace the 64 KiB stdio
 *      buffers of utils/include/buffer.h:61-317 with pinned-host + hipMemcpyAsync staging. ------- */
int ghf_device_alloc(ghf_ctx* ctx, size_t bytes, void** d_ptr);
int ghf_device_free(ghf_ctx* ctx, void* d_ptr);
int ghf_host_alloc(ghf_ctx* ctx, size_t bytes, void** h_ptr); /* pinned */
int ghf_host_free(ghf_ctx* ctx, void* h_ptr);
int ghf_copy_h2d(ghf_ctx* ctx, void* d_dst, const void* h_src, size_t bytes); /* async on the stream */
int ghf_copy_d2h(ghf_ctx* ctx, void* h_dst, const void* d_src, size_t bytes); /* async on the stream */
int ghf_memset_d(ghf_ctx* ctx, void* d_dst, int value, size_t bytes);
/* Device-to-device copy by a kernel with this path's own access shape (16 bytes per lane, four loads in
 * flight, one resident round of workgroups; non_temporal != 0: `global_load/store ... nt`, the hint K1 and K7
 * stream with).  Both pointers 16-byte aligned.  No reference counterpart: it is the bandwidth probe bench.py
 * prices the codec kernels against (what a kernel that only moves the bytes reaches on this box), async on
 * the stream. */
int ghf_copy_d2d(ghf_ctx* ctx, void* d_dst, const void* d_src, size_t bytes, int non_temporal);

/* ---- events: ordering between the streams of several contexts without stopping the host ----------
 * (the file pipeline of golden-huffman_amd/host/glzip_hip.h, which replaces the reference's 64 KiB
 * Buffer, utils/include/buffer.h:61-317, keeps one context per direction: copy-in, kernels, copy-out).
 * record: the event completes when everything enqueued on ctx's stream so far has.  wait: ctx's stream
 * does not run anything enqueued after this call before the event has completed (no host wait).
 * sync: the host waits.  An event that was never recorded counts as complete. */
typedef struct ghf_event ghf_event;
int ghf_event_create(ghf_ctx* ctx, ghf_event** out);
int ghf_event_destroy(ghf_event* ev);
int ghf_event_record(ghf_ctx* ctx, ghf_event* ev);
int ghf_event_wait(ghf_ctx* ctx, ghf_event* ev);
int ghf_event_sync(ghf_event* ev);

/* ---- K1: Encoder::do_init + do_caculate_frequency, include/encoder.h:123-129,136-150 ------------
 * d_hist[0..255] = byte counts of d_in[0..n), d_hist[256] = 1.  d_in needs no alignment (16-byte
 * aligned input takes the fast path).  Also leaves per-chunk histograms in the context so that a
 * following ghf_encode_plan on the same (d_in, n) does not re-read the input -- the caller must not
 * change d_in[0..n) between the two calls. */
int ghf_histogram(ghf_ctx* ctx, const uint8_t* d_in, size_t n, uint64_t* d_hist);
/* The same, for an input that arrives in pieces (the reference counts while it refills its buffer,
 * include/encoder.h:136-150): d_hist[0..255] += byte counts of d_in[0..n), d_hist[256] = 1.  The caller
 * zeroes d_hist (ghf_memset_d) before the first piece.  Keeps nothing for ghf_encode_plan (a piece's
 * buffer is usually refilled in between). */
int ghf_histogram_add(ghf_ctx* ctx, const uint8_t* d_in, size_t n, uint64_t* d_hist);

/* ---- K2+K3: CanonicalHuffEncoder::gen_encode = get_encoding_length + do_gen_encode,
 *      include/canonical_huff_encoder.cc:35-42,289-345,69-141 -- on ONE wavefront, emulating
 *      libstdc++'s priority_queue order exactly.  d_hist is not modified.
 *      The counts' domain: the 257 counts of d_hist must sum to less than 2^GHF_HIST_TOTAL_BITS = 2^55.  A heap entry
 *      is (weight << 9) | symbol index in one 64-bit word -- 9 bits for the 257 indices leave 55 for the weight, and the
 *      root's weight is the sum of all counts -- so beyond that a weight would wrap and the result would be a well-formed
 *      code for other counts.  Such a histogram (ghf_histogram_add and ghf_comm_allreduce_hist accumulate without a limit
 *      of their own; a caller may pass any counts) latches GHF_E_INVAL before anything is built, and d_code is not
 *      written.  The reference counts in 64-bit integers and has no such edge, but no input of fewer than 2^55 - 1 bytes
 *      (32 PiB) reaches it. */
#define GHF_HIST_TOTAL_BITS 55
int ghf_build_code(ghf_ctx* ctx, const uint64_t* d_hist, ghf_code* d_code);

/* ---- a5: CanonicalHuffEncoder::write_encode_info, include/canonical_huff_encoder.cc:210-242 ------
 * Writes the 1040 + 8*max_len header bytes (big-endian u32, utils/include/buffer.h:255-268) at d_out. */
int ghf_write_header(ghf_ctx* ctx, const ghf_code* d_code, uint8_t* d_out, size_t cap);
size_t ghf_header_bytes(int max_len); /* 1040 + 8*max_len */

/* ---- K4 + K5: CanonicalHuffEncoder::encode_file / encode_each_byte,
 *      include/canonical_huff_encoder.cc:245-285 + Buffer::write_bits/write_bit/flush_bits,
 *      utils/include/buffer.h:241-248,277-280,290-295 -- as a two-pass scheme.
 * plan: per-chunk bit totals + exclusive scan; *d_total_bits = sum of code lengths of d_in[0..n)
 *       (the end mark is not included).
 * emit: every wave packs one chunk MSB-first into the pre-sized output.
 *   d_start_bit : absolute stream bit of this buffer's first code (device u64); NULL = right after the
 *                 header, i.e. 8*(1040+8*max_len)  (single-GPU case).
 *   flags       : GHF_EMIT_HEADER the header goes out with the same launches (saves the separate ghf_write_header),
 *                 GHF_EMIT_LAST   append the end mark (symbol 256) and pad with 1-bits to a byte,
 *                 GHF_EMIT_REBASE d_out[0] is stream byte 16*(start_bit/128) instead of stream byte 0
 *                                 (shard-local output buffers of the multi-GPU path).
 *   d_index     : optional side-car for ghf_decode (NULL = none).
 *   d_end       : optional device u64[2] = { absolute end bit of what this call wrote (after padding),
 *                 number of bytes of d_out that are now defined }.
 * Both must be called with the same (d_in, n, d_code); plan first. */
#define GHF_EMIT_LAST 1
#define GHF_EMIT_REBASE 2
#define GHF_EMIT_HEADER 4 /* also write the .crs2 header at d_out[0..) (same bytes as ghf_write_header; not with REBASE) */
#define GHF_EMIT_LONG_CODES 8 /* the tables may hold codes of 33..64 bits (ghf_crs_build_code on a tree deeper than 32:
                                 include/huff_tree.cc:157-170 keeps codes as strings of any length): a second, slower kernel
                                 is queued behind the packer and does the work when the first one finds such a code.  The
                                 canonical format never has them (include/canonical_huff_encoder.h:43-44). */
int ghf_encode_plan(ghf_ctx* ctx, const uint8_t* d_in, size_t n, const ghf_code* d_code, uint64_t* d_total_bits);
int ghf_encode_emit(ghf_ctx* ctx, const uint8_t* d_in, size_t n, const ghf_code* d_code, const uint64_t* d_start_bit,
                    int flags, uint8_t* d_out, size_t cap, const ghf_index* index, uint64_t* d_end);

/* Multi-GPU glue (no reference counterpart: the reference is single-stream): given the all-gathered per-rank body
 * bit totals d_totals[world] (device), *d_start_bit = 8*(1040+8*max_len) + sum of d_totals[0..rank) -- the absolute
 * stream bit at which rank `rank` must start emitting.  One tiny kernel, no host synchronisation. */
int ghf_shard_start_bit(ghf_ctx* ctx, const ghf_code* d_code, const uint64_t* d_totals, int world, int rank,
                        uint64_t* d_start_bit);

/* ---- Compressor<CanonicalHuffEncoder<>>::compress(), include/compressor.h:62-73, in one call:
 *      histogram -> code -> header -> plan -> emit, no host synchronisation in between.
 *      d_out receives the complete .crs2 image; d_out_bytes (device u64) its size. */
int ghf_compress(ghf_ctx* ctx, const uint8_t* d_in, size_t n, uint8_t* d_out, size_t cap, uint64_t* d_out_bytes,
                 ghf_code* d_code /* optional out */, const ghf_index* index /* optional */);
size_t ghf_compress_bound(size_t n); /* capacity that always suffices (Huffman never beats 9 bits/symbol on 257 symbols) */

/* ---- side-car index ------------------------------------------------------------------------------ */
uint32_t ghf_chunk_symbols(size_t n); /* the chunk size the library uses for n input bytes */
int ghf_index_alloc(ghf_ctx* ctx, size_t n_symbols, ghf_index* out);
int ghf_index_free(ghf_ctx* ctx, ghf_index* idx);

/* ---- a7: CanonicalHuffDecoder::get_encode_info, include/canonical_huff_encoder.cc:349-374 (host) -
 * Parses and validates a .crs2 header (the reference trusts it blindly). code->length/codeword are
 * reconstructed from symbol/start_pos/first_code. */
int ghf_parse_header(const uint8_t* h_stream, size_t n, ghf_code* code, size_t* header_bytes);

/* ---- K6/K7: decode_file of CanonicalHuffDecoder / FastCanonicalHuffDecoder /
 *      TableCanonicalHuffDecoder, include/canonical_huff_encoder.cc:377-419,422-461,466-568 ---------
 * d_stream is the buffer an emit call wrote (a whole .crs2 image, or one shard's GHF_EMIT_REBASE buffer)
 * and index the side-car that call filled: the decode is then block-parallel (length-indexed canonical
 * table in LDS).  Without one (index == NULL, e.g. a .crs2 written by the reference; d_stream must then
 * be a whole .crs2 image) the index is first rebuilt on the GPU from the bit stream.  stream_bytes may exceed the
 * stream: the first end mark ends it, as in the reference's decoders (canonical_huff_encoder.cc:404), and what lies
 * behind it is neither decoded nor waited for.
 * d_code may come from anywhere: before anything is decoded the tables are checked on the device to be a
 * complete prefix code (Kraft equality, lengths within [min_len, max_len], first codes that fit their length,
 * start positions inside symbol[]; the one-symbol code of GHF_EMPTY_OK is the exception) -- if not,
 * GHF_E_FORMAT is latched and nothing is written.  Every 64-symbol segment's end is checked against the index
 * (GHF_E_CORRUPT).  A stream whose first code is the end mark decodes to nothing without launching K7.
 * d_out_bytes: device u64 = decoded size. */
int ghf_decode(ghf_ctx* ctx, const uint8_t* d_stream, size_t stream_bytes, const ghf_code* d_code,
               const ghf_index* index, uint8_t* d_out, size_t cap, uint64_t* d_out_bytes);

/* Optional: build the decode tables of d_code ahead of time (one small kernel, k_build_decode_tables) so that the
 * next ghf_decode(..., d_code, index != NULL, ...) on this context starts with the decode kernel itself -- e.g. on
 * another stream while the previous buffer is still being emitted.  Single use: the prepared state is consumed by
 * that ghf_decode and dropped by any other call that rebuilds tables on this context.  The caller orders the two
 * streams (event) and must not change *d_code in between. */
int ghf_decode_prepare(ghf_ctx* ctx, const ghf_code* d_code);

/* Size of what a side-car-less stream decodes to (the .crs2 format does not store it: the reference's
 * decoders simply run until the end mark, include/canonical_huff_encoder.cc:404-411).  Rebuilds the
 * side-car on the GPU, synchronises, and keeps it for a following ghf_decode(index = NULL) of the same
 * (d_stream, stream_bytes), which then does not repeat the work. */
int ghf_decoded_size(ghf_ctx* ctx, const uint8_t* d_stream, size_t stream_bytes, const ghf_code* d_code, uint64_t* n_out);

/* ---- seekable streams: the seek table, the persistent form of the side-car -------------------------
 * No reference counterpart (the .crs2 wire format has no sync points and the reference decodes front to back,
 * include/canonical_huff_encoder.cc:377-568); the .crs2 bytes do not change.  A table is 64 + 24 * ceil(n / 4096)
 * bytes, all fields little-endian: a 64-byte header {"GHFSEEK1", u32 version = 1, u32 flags (GHF_INDEX_NO_END_MARK),
 * u64 n_symbols, u32 block_symbols = 4096, u32 run_symbols = 512, u64 n_blocks, zeros}, then per block of 4096
 * symbols {u64 start_bit (= d_chunk_bit[g]), u16 run_bits[8]: the bit lengths of the block's eight runs of 512
 * symbols, 0 for runs behind the last symbol}.  A block's runs add up to the next block's start_bit minus its own.
 * The caller stores the table where it likes (e.g. <file>.crs2.seek); on open: ghf_seek_parse -> ghf_seek_expand ->
 * ghf_decode with the expanded index, or ghf_decode_range straight from the table. */
typedef struct ghf_seek_info {
  uint64_t n_symbols, n_blocks;
  uint32_t flags, version;
} ghf_seek_info;
size_t ghf_seek_bytes(size_t n_symbols); /* size of the table of a stream of n_symbols (no reference counterpart; host only) */
/* No reference counterpart.  Host only, no GPU, nothing queued: validates the 64-byte header at h_table against
 * `bytes`, the size of the whole table (GHF_E_FORMAT: wrong magic / version / geometry, unknown flags, a size other
 * than the one n_blocks implies -- truncated or with something behind it) and returns its fields. */
int ghf_seek_parse(const uint8_t* h_table, size_t bytes, ghf_seek_info* info);
/* No reference counterpart.  Asynchronous on the stream, never synchronises: the side-car `index` (as an emit call or
 * ghf_seek_expand filled it) -> the table image, header and records, at d_table in DEVICE memory (cap >=
 * ghf_seek_bytes(index->n_symbols), else GHF_E_CAP); the caller brings it to the host with ghf_copy_d2h.
 * index == NULL: the side-car this context last rebuilt for (d_stream, stream_bytes) -- ghf_decoded_size, which DOES
 * synchronise, must have been the last call that rebuilt one; GHF_E_INVAL otherwise: "index a reference-written file
 * once, seek forever".  d_stream is not read.  A side-car whose segment ends do not grow latches GHF_E_CORRUPT. */
int ghf_seek_pack(ghf_ctx* ctx, const ghf_index* index, const uint8_t* d_stream, size_t stream_bytes, uint8_t* d_table,
                  size_t cap);
/* No reference counterpart.  Asynchronous on the stream, never synchronises: the table at d_table (DEVICE memory,
 * table_bytes of it, described by `info` from ghf_seek_parse) -> the full side-car of d_stream in `index`
 * (ghf_index_alloc(info->n_symbols)); index->flags comes from the table.  ghf_decode(..., index, ...) is then the
 * ordinary indexed decode.  One lane per run decodes code lengths only and must land on the run's recorded end, and
 * every block must end where the next one starts: a table that does not fit the stream (or names a bit outside it)
 * latches GHF_E_CORRUPT, a table_bytes other than ghf_seek_bytes(info->n_symbols) is GHF_E_FORMAT at once.  Nothing
 * outside d_stream[0 .. stream_bytes) is read and nothing outside the index arrays written, whatever the table holds.
 * Builds the decode tables of d_code on the context (a state prepared by ghf_decode_prepare is dropped). */
int ghf_seek_expand(ghf_ctx* ctx, const ghf_seek_info* info, const uint8_t* d_table, size_t table_bytes,
                    const uint8_t* d_stream, size_t stream_bytes, const ghf_code* d_code, ghf_index* index);
/* No reference counterpart.  Asynchronous on the stream, never synchronises: d_out[0 .. count) = bytes
 * [first, first + count) of what d_stream decodes to.  Exactly one of `index` (a live side-car) and (info, d_table,
 * table_bytes) (a seek table in DEVICE memory; only the covered blocks are expanded, into a workspace of the context
 * that grows on demand) is given, the other NULL: GHF_E_INVAL otherwise, and for first + count > n_symbols or a
 * misaligned d_stream / d_table.  cap < count: GHF_E_CAP.  count == 0: nothing is launched.  d_out needs no alignment;
 * the decode is fastest when d_out and `first` are congruent modulo 16 (16-byte stores).  Only d_out[0 .. count) is
 * written.  Errors on the device (GHF_E_CORRUPT / GHF_E_FORMAT) are latched as for ghf_decode. */
int ghf_decode_range(ghf_ctx* ctx, const uint8_t* d_stream, size_t stream_bytes, const ghf_code* d_code,
                     const ghf_index* index, const ghf_seek_info* info, const uint8_t* d_table, size_t table_bytes,
                     uint64_t first, uint64_t count, uint8_t* d_out, size_t cap);

/* ---- batches: many small independent .crs2 streams in one call ---------------------------------------
 * No reference counterpart (the reference compresses one file per process, include/compressor.h:62-73).  For callers
 * with thousands of small buffers (pages, records, tensors, log blocks): one call compresses / decodes `count`
 * independent items with ONE kernel launch, whatever `count` is -- one workgroup per item, which histograms, builds the
 * exact code (the same K2/K3 body ghf_build_code runs), packs and writes the header.  Asynchronous on the context's
 * stream, never synchronises, no per-item host work or copy: EVERY array argument, the pointer and size arrays
 * included, is DEVICE memory; the host knows `count` and `max_item_bytes` only.
 *
 * Compress: item i = d_in_ptrs[i][0 .. d_in_bytes[i]) -> a complete standalone .crs2 image at d_out_ptrs[i],
 * byte-identical to what ghf_compress writes for the same bytes (and so to the reference's file); d_out_bytes[i] <- its
 * size.  Bytes behind the image are unspecified; nothing at or beyond d_out_caps[i] is written
 * (ghf_compress_batch_bound(max_item_bytes) always suffices).  Input pointers need no alignment; compress output
 * pointers and decode stream pointers are 16-byte aligned; decode output pointers need no alignment.  d_codes
 * (optional): d_codes[i] <- the tables ghf_build_code produces.  index (optional): item i's slice receives exactly the
 * side-car ghf_compress(..., index) fills for that item; chunk_bit counts from byte 0 of the item's own image.
 *
 * Decode: item i = the image at d_stream_ptrs[i] (d_stream_bytes[i] of it), with d_codes[i], item i's slice of `index`
 * and d_n_symbols[i] (what the compress call was given) -> d_out_ptrs[i][0 .. d_n_symbols[i]), d_out_bytes[i] <- that
 * size.  The tables pass the checks of ghf_decode (complete prefix code) before anything is decoded; every segment must
 * land on its recorded end and the end mark must follow the last symbol.  No byte outside d_stream_ptrs[i][0 ..
 * d_stream_bytes[i]) is read, whatever tables and side-car hold.  Streams without side-car, tables or sizes (files the
 * reference wrote, stored images of ghf_compress_batch) go through ghf_decode_images_batch below; one large stream
 * through ghf_decode(index = NULL).
 *
 * Failures are PER ITEM: d_item_status[i] <- a ghf_status_code (GHF_OK is written as well):
 *   GHF_E_EMPTY   the item has 0 bytes            GHF_E_INVAL  more than max_item_bytes; null / misaligned item pointer
 *   GHF_E_CAP     the image (the decoded item) is larger than d_out_caps[i]
 *   GHF_E_FORMAT  decode: d_codes[i] is not a complete prefix code
 *   GHF_E_CORRUPT decode: a segment does not land on its recorded end, or the end mark is missing / cut off
 * A failed item leaves d_out_bytes[i] = 0, does not disturb its neighbours and does NOT latch the context's status word:
 * ghf_sync stays GHF_OK.  Call-level errors (returned at once, nothing queued): null arrays, max_item_bytes == 0 or
 * > GHF_BATCH_MAX_ITEM, an index whose geometry does not cover (count, max_item_bytes): GHF_E_INVAL.  count == 0 queues
 * nothing.  The calls leave the context's plan, histogram and prepared-table caches alone.
 * Not supported here: GHF_CODE_LIMIT and GHF_EMPTY_OK (a code longer than 32 bits needs far more than 1 MiB of input;
 * an empty item is refused), and the .crs format. */
#define GHF_BATCH_MAX_ITEM (1u << 20) /* one workgroup owns one item; its bit offsets fit 32 bits */

/* No reference counterpart.  Host only: = ghf_compress_bound(max_item_bytes), a capacity that suffices for every item. */
size_t ghf_compress_batch_bound(size_t max_item_bytes);

/* The side-cars of a batch: a host struct with two device arrays; item i's slice is the SAME side-car ghf_index
 * describes, at a fixed stride. */
typedef struct ghf_batch_index {
  uint32_t count, reserved;
  uint64_t max_item_bytes;
  uint64_t blocks_per_item; /* ceil(max_item_bytes / 4096) */
  uint64_t segs_per_item;   /* ceil(max_item_bytes / 64) */
  uint64_t* d_chunk_bit;    /* [count * blocks_per_item], item i at i * blocks_per_item */
  uint32_t* d_seg_bit;      /* [count * segs_per_item],   item i at i * segs_per_item */
} ghf_batch_index;
/* No reference counterpart.  Allocates the two arrays for `count` items of up to max_item_bytes (<= GHF_BATCH_MAX_ITEM). */
int ghf_batch_index_alloc(ghf_ctx* ctx, uint32_t count, size_t max_item_bytes, ghf_batch_index* out);
/* No reference counterpart.  Waits for the context's stream, then frees the arrays. */
int ghf_batch_index_free(ghf_ctx* ctx, ghf_batch_index* idx);
/* No reference counterpart.  Host only, nothing queued: item i's slice as an ordinary ghf_index (n_symbols = n_i, the
 * item's size) -- usable with ghf_decode, ghf_seek_pack and ghf_decode_range on the item's image.  The view owns
 * nothing (do not ghf_index_free it).  GHF_E_INVAL: i >= count, n_i > max_item_bytes. */
int ghf_batch_index_item(const ghf_batch_index* idx, uint32_t i, size_t n_i, ghf_index* view);

/* No reference counterpart; see above. */
int ghf_compress_batch(ghf_ctx* ctx, const uint8_t* const* d_in_ptrs, const uint64_t* d_in_bytes, size_t max_item_bytes,
                       uint32_t count, uint8_t* const* d_out_ptrs, const uint64_t* d_out_caps, uint64_t* d_out_bytes,
                       ghf_code* d_codes /* [count], optional */, const ghf_batch_index* index /* optional */,
                       int* d_item_status /* [count] */);
/* No reference counterpart; see above.  max_item_bytes is index->max_item_bytes. */
int ghf_decode_batch(ghf_ctx* ctx, const uint8_t* const* d_stream_ptrs, const uint64_t* d_stream_bytes,
                     const ghf_code* d_codes /* [count] */, const ghf_batch_index* index, const uint64_t* d_n_symbols,
                     uint32_t count, uint8_t* const* d_out_ptrs, const uint64_t* d_out_caps, uint64_t* d_out_bytes,
                     int* d_item_status /* [count] */);

/* No reference counterpart (the reference decodes one file per process, include/compressor.h:87-92).
 * Decode `count` standalone .crs2 images that come with nothing else -- files the reference wrote, or images of
 * ghf_compress_batch whose tables and side-car are gone.  ONE launch, one workgroup per item, asynchronous on the
 * context's stream, never synchronises; every array is DEVICE memory.
 * d_out_ptrs == NULL (then d_out_caps is ignored): sizes only -- d_out_bytes[i] <- what item i decodes to.
 *
 * Item i = the image at d_stream_ptrs[i] (16-byte aligned), d_stream_bytes[i] of it.  The header is parsed on the device
 * with every check ghf_parse_header makes; the body is decoded from bit 8 * (1040 + 8 * max_len) until the first end
 * mark, as ghf_decode does: d_stream_bytes[i] may exceed the stream, what lies behind the end mark is not decoded.  The
 * result goes to d_out_ptrs[i][0 .. n_i) (no alignment needed), d_out_bytes[i] <- n_i.  On success only d_out[0 .. n_i)
 * is written; on failure nothing at or beyond d_out_caps[i] is written and d_out_bytes[i] = 0.  No byte outside
 * d_stream_ptrs[i][0 .. d_stream_bytes[i]) is ever read, whatever the header says.  d_codes[i] (optional) receives
 * exactly what ghf_parse_header returns for the same header (untouched when the item fails before its header is
 * accepted).  The one-symbol image of GHF_EMPTY_OK (1049 bytes) is accepted and decodes to nothing: GHF_OK, 0 bytes.
 *
 * d_item_status[i] <- (GHF_OK is written as well)
 *   GHF_E_INVAL   null or misaligned stream pointer; null output pointer in decode mode; d_stream_bytes[i] greater than
 *                 ghf_compress_bound(GHF_BATCH_MAX_ITEM)
 *   GHF_E_FORMAT  ghf_parse_header would refuse the header (a stream shorter than its header included)
 *   GHF_E_CAP     the item decodes to more than d_out_caps[i] (sizes only: the true count is reported with GHF_OK)
 *   GHF_E_CORRUPT the stream ends before a whole end mark has been found (with a complete prefix code the only
 *                 corruption any decoder can see)
 * As in the other batch calls failures are per item and never latch the context's status word.  Call-level errors
 * (returned at once, nothing queued): null d_stream_ptrs / d_stream_bytes / d_out_bytes / d_item_status, d_out_ptrs
 * without d_out_caps: GHF_E_INVAL.  count == 0 queues nothing.  The context's plan, histogram, prepared-table and K6
 * caches are left alone.
 * The workgroup finds the code boundaries itself, in rounds of 256 subsequences of 512 bits that settle in at most 256
 * passes each: codes that barely self-synchronise (8/9-bit codes of uniform bytes) cost up to
 * one lane decoding the item front to back. */
int ghf_decode_images_batch(ghf_ctx* ctx, const uint8_t* const* d_stream_ptrs, const uint64_t* d_stream_bytes,
                            uint32_t count, uint8_t* const* d_out_ptrs, const uint64_t* d_out_caps,
                            uint64_t* d_out_bytes, ghf_code* d_codes /* [count], optional OUT */,
                            int* d_item_status /* [count] */);
/* No reference counterpart.  Host only, nothing queued: d_stats (device u64[2], 8-byte aligned; NULL, the default:
 * nowhere) -- every later ghf_decode_images_batch on this context adds, over all items that reached their body,
 * d_stats[0] += rounds and d_stats[1] += passes.  The caller zeroes the two words; tools/batch_images_bench.py reads
 * them to hold the observed passes per round against the bound of 256.  ghf_decode_bodies_batch_shared (below) runs the
 * same rounds and passes and adds its own to the same two words. */
int ghf_decode_images_batch_stats(ghf_ctx* ctx, uint64_t* d_stats);

/* ---- shared-code batches: one code for many small items ---------------------------------------------
 * No reference counterpart (the reference compresses one file per process, include/compressor.h:62-73).  The batch calls
 * above give every item a code of its own: 1040 + 8 * max_len bytes of header per image and 3604 bytes of tables per
 * item for the decoder -- as much as a 4 KiB item itself.  These calls put ONE code under the whole batch.  The header is
 * stored once; item i's output is its BODY alone: the codes of its bytes MSB-first from bit 0, the end mark, 1-bits up
 * to the byte -- exactly the bytes ghf_encode_emit writes for (d_in, n, d_code, a device start bit of 0, GHF_EMIT_LAST).
 * The .crs2 format does not change: a body is byte-aligned behind its header, so header(code) || body(i) (the header
 * from ghf_write_header) is a complete standalone .crs2 image that the reference's decoders, ghf_decode and
 * ghf_decode_images_batch read.
 *
 * Conventions are those of the batch calls above: every array is DEVICE memory; asynchronous on the context's stream,
 * never synchronises; failures are per item (GHF_OK is written as well, d_out_bytes[i] = 0 on failure) and never latch
 * the context's status word; the context's caches are left alone; count == 0 queues nothing.  Call-level errors (returned
 * at once, nothing queued): null arrays, max_item_bytes == 0 or > GHF_BATCH_MAX_ITEM, an index whose geometry does not
 * cover (count, max_item_bytes), unknown flags, a null or not 16-byte aligned d_code: GHF_E_INVAL.  Input and decode-output
 * pointers need no alignment; compress-output and decode-stream pointers are 16-byte aligned.
 *
 * The code: ghf_build_code or ghf_build_code_ex(GHF_CODE_LIMIT) on the histogram of ghf_histogram_batch, or any other
 * ghf_code in device memory (one trained on a sample; one from ghf_parse_header, copied up).  Both kernels check it
 * before they trust it: a d_code that is not a complete prefix code of lengths <= 32 with a code for the end mark (the
 * rules ghf_decode_batch applies to an item's tables) gives GHF_E_FORMAT on EVERY item, and nothing is written.
 * Bodies whose side-car and sizes are gone (stored bodies, read back by another process) go through
 * ghf_decode_bodies_batch_shared below.  Not supported here: GHF_EMPTY_OK items, and the .crs format. */
#define GHF_HIST_COVER_ALL 1u /* ghf_histogram_batch: every count of 0 becomes 1 */

/* No reference counterpart; see above.  d_hist[0..255] <- the byte counts summed over all items, d_hist[256] <- 1: what
 * ghf_histogram gives for the items' concatenation.  d_hist (device u64[257]) is overwritten, the caller zeroes nothing.
 * Items of 0 bytes, with a null pointer or of more than max_item_bytes contribute nothing (ghf_compress_batch_shared is
 * what reports them).  GHF_HIST_COVER_ALL: every count of 0 becomes 1, so the code built from the result has a code
 * for every byte value and later items compress whatever they hold. */
int ghf_histogram_batch(ghf_ctx* ctx, const uint8_t* const* d_in_ptrs, const uint64_t* d_in_bytes, size_t max_item_bytes,
                        uint32_t count, unsigned flags, uint64_t* d_hist /* [257] */);

/* No reference counterpart.  Host only: (4 * max_item_bytes + 4 + 15) & ~15, a capacity that suffices for the body of
 * every item under any code of <= 32 bits. */
size_t ghf_compress_batch_shared_bound(size_t max_item_bytes);

/* No reference counterpart; see above.  Item i = d_in_ptrs[i][0 .. d_in_bytes[i]) -> its body at d_out_ptrs[i],
 * d_out_bytes[i] <- its size.  Nothing at or beyond d_out_caps[i] is written, and a refused item writes nothing at all:
 * the size is known from a pricing pass before the first store.  index (optional): item i's slice receives the side-car
 * of that body; chunk_bit counts from byte 0 of the body, a segment end is relative to its block.
 * d_item_status[i] <-
 *   GHF_E_EMPTY   the item has 0 bytes            GHF_E_INVAL  more than max_item_bytes; null / misaligned item pointer
 *   GHF_E_CAP     the body is larger than d_out_caps[i]
 *   GHF_E_NOCODE  the item holds a byte value to which d_code gives no code
 *   GHF_E_FORMAT  (every item) d_code is not a complete prefix code */
int ghf_compress_batch_shared(ghf_ctx* ctx, const uint8_t* const* d_in_ptrs, const uint64_t* d_in_bytes,
                              size_t max_item_bytes, uint32_t count, const ghf_code* d_code, uint8_t* const* d_out_ptrs,
                              const uint64_t* d_out_caps, uint64_t* d_out_bytes,
                              const ghf_batch_index* index /* optional */, int* d_item_status /* [count] */);

/* No reference counterpart; see above.  ghf_decode_batch with one d_code for all items and bodies that start at bit 0:
 * item i = the body at d_stream_ptrs[i] (d_stream_bytes[i] of it), item i's slice of `index` and d_n_symbols[i] ->
 * d_out_ptrs[i][0 .. d_n_symbols[i]).  max_item_bytes is index->max_item_bytes.  Every segment must land on its recorded
 * end and the end mark must follow the last symbol (GHF_E_CORRUPT); GHF_E_CAP, GHF_E_EMPTY, GHF_E_INVAL as in
 * ghf_decode_batch; GHF_E_FORMAT (every item) for a d_code that is not a complete prefix code.  No byte outside
 * d_stream_ptrs[i][0 .. d_stream_bytes[i]) is read, whatever code and side-car hold. */
int ghf_decode_batch_shared(ghf_ctx* ctx, const uint8_t* const* d_stream_ptrs, const uint64_t* d_stream_bytes,
                            const ghf_code* d_code, const ghf_batch_index* index, const uint64_t* d_n_symbols,
                            uint32_t count, uint8_t* const* d_out_ptrs, const uint64_t* d_out_caps,
                            uint64_t* d_out_bytes, int* d_item_status /* [count] */);

/* No reference counterpart; see above.  ghf_decode_images_batch for bodies under one code: the fourth corner of
 * {a code per item, one shared code} x {live side-car, nothing but the bytes}.  No side-car, no sizes and no per-item
 * tables are passed.  ONE launch whatever count is, one workgroup per item.
 * d_out_ptrs == NULL (then d_out_caps is ignored): sizes only -- d_out_bytes[i] <- what item i decodes to.
 *
 * Item i = the body at d_stream_ptrs[i] (16-byte aligned), d_stream_bytes[i] of it.  The body is decoded from bit 0 until
 * the first end mark: d_stream_bytes[i] may exceed the body, what lies behind the end mark is not decoded.  The result
 * goes to d_out_ptrs[i][0 .. n_i) (no alignment needed), d_out_bytes[i] <- n_i.  On success only d_out[0 .. n_i) is
 * written; on failure nothing at or beyond d_out_caps[i] is written and d_out_bytes[i] = 0.  No byte outside
 * d_stream_ptrs[i][0 .. d_stream_bytes[i]) is ever read, whatever the code holds.  A body whose first code is the end
 * mark decodes to nothing: GHF_OK, 0 bytes (as in ghf_decode and ghf_decode_images_batch).
 *
 * The code is vetted before any item is looked at, with the rules ghf_decode_batch_shared applies: a d_code that is not a
 * complete prefix code of lengths <= 32 gives GHF_E_FORMAT on EVERY item, and nothing is written.  The lone-end-mark code
 * of GHF_EMPTY_OK is not complete and is refused the same way.
 *
 * d_item_status[i] <- (GHF_OK is written as well)
 *   GHF_E_INVAL   null or misaligned stream pointer; null output pointer in decode mode; d_stream_bytes[i] greater than
 *                 ghf_compress_batch_shared_bound(GHF_BATCH_MAX_ITEM) (every bit offset then fits 32 bits)
 *   GHF_E_CAP     the item decodes to more than d_out_caps[i]; checked before any store of the round that would cross it
 *                 (sizes only: the true count is reported with GHF_OK)
 *   GHF_E_CORRUPT the stream ends before a whole end mark has been found; d_stream_bytes[i] == 0 is this case
 *   GHF_E_FORMAT  (every item) d_code is not a complete prefix code
 * Call-level errors (returned at once, nothing queued): null d_stream_ptrs / d_stream_bytes / d_out_bytes /
 * d_item_status, d_out_ptrs without d_out_caps, a null or not 16-byte aligned d_code: GHF_E_INVAL.
 * The workgroup finds the code boundaries itself, in the rounds and passes of ghf_decode_images_batch (DESIGN.md sections
 * 10 and 13); the words named by ghf_decode_images_batch_stats receive this call's rounds and passes too. */
int ghf_decode_bodies_batch_shared(ghf_ctx* ctx, const uint8_t* const* d_stream_ptrs, const uint64_t* d_stream_bytes,
                                   const ghf_code* d_code, uint32_t count, uint8_t* const* d_out_ptrs,
                                   const uint64_t* d_out_caps, uint64_t* d_out_bytes, int* d_item_status /* [count] */);

/* ---- byte planes: typed elements (bf16 / fp32 / 64-bit) as one .crs2 image per byte position --------
 * No reference counterpart (the reference compresses one flat run of bytes per process, include/compressor.h:62-73, and
 * reads one back, include/compressor.h:87-92).  Callers that hold elements of 2, 4 or 8 bytes lose most of the skew of the
 * high (sign / exponent) byte when all bytes share one histogram.  These calls split the elements into elem_bytes PLANES
 * -- plane b holds byte b of every element, in element order (the "shuffle" filter of Blosc, ZipNN and HDF5) -- and
 * compress every plane by itself.  The .crs2 format does not change: EACH PLANE IS AN ORDINARY STANDALONE .crs2 IMAGE of
 * the bytes d_in[b], d_in[b + E], d_in[b + 2 E] ..., byte-identical to what ghf_compress (and so the reference) writes for
 * them; the reference's decoders, ghf_decode, the seek table and ghf_decode_range read it as any other.
 *
 * elem_bytes is 2, 4 or 8.  Every device pointer is 16-byte aligned and so are plane_stride and slot_bytes.  These
 * call-level errors are returned at once with nothing queued, checked before anything touches HIP: a null context or
 * required pointer, another elem_bytes, a misaligned pointer / plane_stride / slot_bytes, n_elems * elem_bytes beyond
 * size_t, an indexes[p] that does not cover n_elems: GHF_E_INVAL; then n_elems == 0: GHF_E_EMPTY; then plane_stride <
 * n_elems, slot_bytes < ghf_planes_slot_bytes(n_elems), cap < n_elems * elem_bytes: GHF_E_CAP.  "Nothing queued" holds for
 * these conditions only: whatever else an inner ghf_compress / ghf_decoded_size / ghf_decode refuses for one plane (a
 * stream shorter than its header, an allocation that fails) is returned when that plane is reached, behind the split and
 * the planes queued before it; d_out of ghf_decode_planes is still untouched then, the merge comes last. */
#define GHF_PLANES_MAX 8

/* No reference counterpart.  Host only: (ghf_compress_bound(n_elems) + 15) & ~15, a slot that suffices for any plane of
 * n_elems bytes. */
size_t ghf_planes_slot_bytes(size_t n_elems);

/* No reference counterpart (generalises the flat input of include/compressor.h:62-73).  Asynchronous on the stream, never
 * synchronises: byte b of element k of d_in[0 .. n_elems * elem_bytes) goes to d_planes[b * plane_stride + k].  Only
 * [0, n_elems) of every plane is written.  One streaming kernel: 16 bytes per lane on both sides, the transposition in
 * registers and a wave-private LDS tile. */
int ghf_planes_split(ghf_ctx* ctx, const uint8_t* d_in, size_t n_elems, uint32_t elem_bytes, uint8_t* d_planes,
                     size_t plane_stride);
/* No reference counterpart (generalises the flat output of include/compressor.h:87-92).  The inverse of ghf_planes_split:
 * only d_out[0 .. n_elems * elem_bytes) is written.  Does not look at the context's status word. */
int ghf_planes_merge(ghf_ctx* ctx, const uint8_t* d_planes, size_t plane_stride, size_t n_elems, uint32_t elem_bytes,
                     uint8_t* d_out);

/* No reference counterpart: Compressor::compress(), include/compressor.h:62-73, once per byte plane.  Asynchronous on the
 * stream, no host synchronisation: splits d_in into a workspace of the context that grows on demand, then does for
 * p = 0 .. elem_bytes - 1 exactly what ghf_compress does for plane p: the image goes to d_out + p * slot_bytes, its size to
 * d_out_bytes[p] (device u64[elem_bytes]); d_codes[p] (device, optional) and indexes[p] (a HOST array of elem_bytes
 * side-cars, each from ghf_index_alloc(n_elems); optional) are filled as ghf_compress fills d_code and index.  Device-side
 * failures latch as for ghf_compress.  An indexes[p] that was not allocated for n_elems: GHF_E_INVAL, nothing queued. */
int ghf_compress_planes(ghf_ctx* ctx, const uint8_t* d_in, size_t n_elems, uint32_t elem_bytes, uint8_t* d_out,
                        size_t slot_bytes, uint64_t* d_out_bytes, ghf_code* d_codes, const ghf_index* indexes);

/* No reference counterpart: Decompressor::decompress(), include/compressor.h:87-92, once per byte plane.  ghf_decode of
 * plane p = the image at h_stream_ptrs[p] (a HOST array of elem_bytes device pointers), h_stream_bytes[p] (HOST) of it,
 * with d_codes[p] (device) and indexes[p], into the context's workspace; then the merge into d_out[0 .. n_elems *
 * elem_bytes), d_out_bytes (device u64, optional) <- that size.
 * indexes != NULL (a HOST array of elem_bytes side-cars): the call never synchronises.  Every indexes[p].n_symbols must
 * equal n_elems: GHF_E_INVAL otherwise, nothing queued.
 * indexes == NULL: every plane takes the side-car-less path, which SYNCHRONISES with the host as ghf_decoded_size and
 * ghf_decode(index = NULL) do.  A plane that decodes to another size than n_elems: GHF_E_CORRUPT is returned and no merge
 * is queued (d_out is untouched).
 * The merge does not run on the planes of a failed decode: a launch that finds the context's latched status non-zero stores
 * nothing (the convention of the decode kernel itself); ghf_sync reports the status. */
int ghf_decode_planes(ghf_ctx* ctx, const uint8_t* const* h_stream_ptrs, const size_t* h_stream_bytes,
                      const ghf_code* d_codes, const ghf_index* indexes, size_t n_elems, uint32_t elem_bytes, uint8_t* d_out,
                      size_t cap, uint64_t* d_out_bytes);

/* ---- byte planes in stages: the plane histograms of one large typed buffer in one pass, what
 * it would compress to, and compression under codes the caller brings.  Conventions and call-level errors are those of
 * the byte-plane calls above. */

/* No reference counterpart (generalises the flat count of include/encoder.h:123-150, which include/compressor.h:62-73
 * runs once per file).  Asynchronous on the stream, never synchronises; one pass over d_in[0 .. n_elems * elem_bytes),
 * nothing behind it is read: d_hists[p][0 .. 255] (device u64[elem_bytes][257], overwritten) <- the counts of the bytes
 * d_in[p], d_in[p + E], ..., exactly what ghf_histogram gives for plane p of ghf_planes_split; d_hists[p][256] = 1.  flags:
 * GHF_HIST_COVER_ALL, honoured per plane.  Leaves the context's caches alone.  A null context or pointer, another
 * elem_bytes, d_in not 16-byte aligned, unknown flags, n_elems * elem_bytes beyond size_t: GHF_E_INVAL; then n_elems == 0:
 * GHF_E_EMPTY; nothing queued. */
int ghf_histogram_planes(ghf_ctx* ctx, const uint8_t* d_in, size_t n_elems, uint32_t elem_bytes, unsigned flags,
                         uint64_t* d_hists /* [elem_bytes][257] */);

/* No reference counterpart (include/compressor.h:62-73 learns a file's compressed size by compressing it; the sum is
 * the one include/encoder.h:123-150 would make over the counts).  Asynchronous, never synchronises, one tiny launch:
 * d_bytes[p] (device u64[elem_bytes]) <- ghf_header_bytes(max_len of d_codes[p]) + ceil((sum over b < 256 of d_hists[p][b] *
 * length_p[b] + length_p[256]) / 8), the exact size of the image any compress call writes for a plane with these counts
 * under that code; 0 when d_codes[p] is not a complete prefix code or gives no code to a byte with a non-zero count (or
 * to the end mark).  Latches nothing, leaves the context's caches alone.  A null context or pointer, another elem_bytes:
 * GHF_E_INVAL. */
int ghf_planes_image_bytes(ghf_ctx* ctx, const uint64_t* d_hists /* [elem_bytes][257] */, const ghf_code* d_codes,
                           uint32_t elem_bytes, uint64_t* d_bytes /* [elem_bytes] */);

/* No reference counterpart: Compressor::compress(), include/compressor.h:62-73, once per byte plane, with its count
 * (include/encoder.h:123-150) made for all planes in one pass and its code either built for all planes in one launch or
 * brought by the caller.  Arguments, their checks and the order of the checks are ghf_compress_planes'; in addition d_codes
 * (device, [elem_bytes]) is required -- null or not 16-byte aligned: GHF_E_INVAL -- and unknown flags are GHF_E_INVAL.
 * Asynchronous on the stream, never synchronises.  On the stream: ghf_histogram_planes into counters of the context; the
 * codes (below); ghf_planes_split into the context's workspace; per plane ghf_encode_plan and ghf_encode_emit(GHF_EMIT_HEADER |
 * GHF_EMIT_LAST, indexes[p]) into d_out + p * slot_bytes, d_out_bytes[p] <- the image's size.  The plan and histogram caches
 * of the context are forgotten, as by ghf_compress_planes.
 * GHF_PLANES_BUILD_CODES: d_codes is OUT, filled by one ghf_build_codes launch from the counts; every image, size, code and
 * side-car is then byte for byte what ghf_compress_planes writes.
 * Without it d_codes is IN (trained on another tensor, parsed from a stored header): plane p's image is
 * ghf_write_header(d_codes + p) followed by the body under that code, an ordinary .crs2 that the reference, ghf_decode,
 * ghf_decode_planes, the seek table and the range calls read.  The codes are vetted on the device first: one that is not a
 * complete prefix code latches GHF_E_FORMAT on the context's status word, a plane that holds a byte value to which its code
 * gives no code latches GHF_E_NOCODE (train with GHF_HIST_COVER_ALL to rule that out).
 * A latched status stops everything behind it: nothing reaches d_out, d_out_bytes is UNSPECIFIED; ghf_sync reports the
 * status and ghf_clear_status makes the context usable again. */
#define GHF_PLANES_BUILD_CODES 1u
int ghf_compress_planes_coded(ghf_ctx* ctx, const uint8_t* d_in, size_t n_elems, uint32_t elem_bytes,
                              ghf_code* d_codes /* [elem_bytes] 16-byte aligned: in or out with BUILD_CODES */, unsigned flags,
                              uint8_t* d_out, size_t slot_bytes, uint64_t* d_out_bytes, const ghf_index* indexes);

/* ---- shared-code batches of typed elements: one code per byte plane for many small items -------------
 * No reference counterpart (the reference compresses one flat run of bytes per process, include/compressor.h:62-73, and
 * reads one back, include/compressor.h:87-92).  The shared-code batch calls put one code under thousands of small flat
 * items; the byte-plane calls give the byte positions of ONE large buffer a code each.  These calls do both: an item is a
 * run of elements of elem_bytes = E (2, 4 or 8) bytes, plane p of it is the bytes in[p], in[p + E], in[p + 2 E] ..., and
 * ONE code per plane lies under the whole batch.  The planes are never materialised.  The .crs2 format does not change:
 * "slot" j = i * E + p names (item i, plane p); its output is the BODY that ghf_compress_batch_shared writes for the
 * plane's bytes under d_codes[p], so ghf_write_header(d_codes + p) || body(j) is a standalone .crs2 image of the plane that
 * the reference's decoders, ghf_decode and ghf_decode_images_batch read.
 *
 * Conventions are those of the shared-code batch calls: every array is DEVICE memory; asynchronous on the context's
 * stream, never synchronises; failures are per slot or per item and never latch the context's status word (ghf_build_codes
 * latches as ghf_build_code_ex does); the context's caches are left alone (ghf_build_codes forgets what was derived from
 * the codes it overwrites, as ghf_build_code_ex does); count == 0 queues nothing.  Call-level errors
 * (returned at once, nothing queued, checked before anything touches HIP): a null context or array, an elem_bytes other
 * than 2, 4 or 8, max_item_bytes == 0, > GHF_BATCH_MAX_ITEM or not a multiple of elem_bytes, an index whose geometry does
 * not cover (count * elem_bytes, max_item_bytes / elem_bytes), unknown flags, null or not 16-byte aligned d_codes:
 * GHF_E_INVAL. */

/* No reference counterpart (include/compressor.h:62-73 counts one flat run; 87-92 reads one back).  One pass over the
 * items: d_hists[p] (device u64[elem_bytes][257], overwritten) <- what ghf_histogram_batch gives for the items' plane-p
 * bytes, slot 256 = 1, GHF_HIST_COVER_ALL honoured per plane.  Items of 0 bytes, with a null pointer, of more than
 * max_item_bytes or whose size is not a multiple of elem_bytes contribute nothing (ghf_compress_batch_planes_shared
 * reports them). */
int ghf_histogram_batch_planes(ghf_ctx* ctx, const uint8_t* const* d_in_ptrs, const uint64_t* d_in_bytes,
                               size_t max_item_bytes, uint32_t count, uint32_t elem_bytes, unsigned flags,
                               uint64_t* d_hists /* [elem_bytes][257] */);

/* No reference counterpart (include/compressor.h:62-73 builds one code per file; 87-92 reads one).  n_codes (1 ..
 * GHF_PLANES_MAX) exact code builds in ONE launch: d_codes[k] is bit-identical to what ghf_build_code_ex(d_hists + 257 k,
 * d_codes + k, flags) leaves, and device failures latch exactly as there.  As there too, and unlike the other calls of
 * this group, it touches the context's caches: what the context derived from the former contents of one of d_codes (the
 * plan or the prepared tables of a ghf_compress / ghf_decode under that code) is forgotten, since the tables change.
 * Every histogram is held to the counts' domain stated at ghf_build_code (sum below 2^GHF_HIST_TOTAL_BITS): one that is
 * not latches GHF_E_INVAL and leaves its d_codes[k] unwritten, the other codes of the launch are built as usual.
 * n_codes == 0 or > GHF_PLANES_MAX: GHF_E_INVAL. */
int ghf_build_codes(ghf_ctx* ctx, const uint64_t* d_hists /* [n_codes][257] */, uint32_t n_codes,
                    ghf_code* d_codes /* [n_codes] */, unsigned flags);

/* No reference counterpart (include/compressor.h:62-73, 87-92).  Host only: ghf_compress_batch_shared_bound(max_item_bytes
 * / elem_bytes), a capacity that suffices for every slot under any code of <= 32 bits; 0 for another elem_bytes. */
size_t ghf_compress_batch_planes_shared_bound(size_t max_item_bytes, uint32_t elem_bytes);

/* No reference counterpart (generalises include/compressor.h:62-73; 87-92 is the way back).  Item i = d_in_ptrs[i][0 ..
 * d_in_bytes[i]) (no alignment needed); slot j = i * elem_bytes + p receives the body of plane p under d_codes[p]
 * (device ghf_code[elem_bytes], 16-byte aligned) at d_out_ptrs[j] (16-byte aligned), d_out_bytes[j] <- its size: byte for
 * byte what ghf_compress_batch_shared writes for the plane's bytes.  Nothing at or beyond d_out_caps[j] is written, and a
 * refused slot writes nothing.  index (optional): a ghf_batch_index allocated for count * elem_bytes items of
 * max_item_bytes / elem_bytes; slice j receives the side-car ghf_compress_batch_shared would fill for that plane.
 * d_item_status[j] <- as ghf_compress_batch_shared (GHF_E_EMPTY, GHF_E_INVAL, GHF_E_CAP, GHF_E_NOCODE per slot), and
 *   GHF_E_INVAL   on all elem_bytes slots of an item whose size is not a multiple of elem_bytes
 *   GHF_E_FORMAT  only on the slots of a plane whose code is not a complete prefix code */
int ghf_compress_batch_planes_shared(ghf_ctx* ctx, const uint8_t* const* d_in_ptrs, const uint64_t* d_in_bytes,
                                     size_t max_item_bytes, uint32_t count, uint32_t elem_bytes, const ghf_code* d_codes,
                                     uint8_t* const* d_out_ptrs, const uint64_t* d_out_caps, uint64_t* d_out_bytes,
                                     const ghf_batch_index* index /* optional */, int* d_item_status /* [count * elem_bytes] */);

/* No reference counterpart (include/compressor.h:62-73 is the way there; generalises 87-92).  The bodies of
 * ghf_compress_batch_planes_shared with their live side-car: slot j = the body at d_stream_ptrs[j] (16-byte aligned),
 * d_stream_bytes[j] of it, and slice j of `index`.  Output and status are PER ITEM: byte p of element k of item i goes to
 * d_out_ptrs[i][k * elem_bytes + p] (no alignment needed), d_out_bytes[i] <- d_n_elems[i] * elem_bytes; d_out_caps[i] is in
 * bytes.  Every plane passes the segment-end and end-mark checks of ghf_decode_batch_shared.  d_item_status[i] <-
 * GHF_E_EMPTY (0 elements), GHF_E_INVAL (more elements than a slice of the index covers; a null or misaligned stream
 * pointer of any plane; a null output pointer), GHF_E_CAP, GHF_E_CORRUPT; GHF_E_FORMAT on EVERY item if any of the
 * elem_bytes codes is not a complete prefix code, and nothing is written. */
int ghf_decode_batch_planes_shared(ghf_ctx* ctx, const uint8_t* const* d_stream_ptrs, const uint64_t* d_stream_bytes,
                                   const ghf_code* d_codes, const ghf_batch_index* index, const uint64_t* d_n_elems,
                                   uint32_t count, uint32_t elem_bytes, uint8_t* const* d_out_ptrs,
                                   const uint64_t* d_out_caps, uint64_t* d_out_bytes, int* d_item_status /* [count] */);

/* No reference counterpart (include/compressor.h:62-73 is the way there; generalises 87-92).  ghf_decode_bodies_batch_shared
 * for the slots of ghf_compress_batch_planes_shared: nothing but the bytes, no side-car, no sizes.  d_out_ptrs == NULL
 * (then d_out_caps is ignored): sizes only.  Each plane of item i is decoded from bit 0 to its first end mark and written
 * as in ghf_decode_batch_planes_shared; d_out_bytes[i] <- n_i * elem_bytes.  d_item_status[i] <-
 *   GHF_E_INVAL   as ghf_decode_bodies_batch_shared, for any plane of the item
 *   GHF_E_CORRUPT a plane's stream ends before a whole end mark; the planes decode to different numbers of symbols
 *   GHF_E_CAP     n_i * elem_bytes > d_out_caps[i]: a plane's cap is d_out_caps[i] / elem_bytes symbols, checked before any
 *                 store of the round that would cross it; nothing at or beyond d_out_caps[i] is written
 *   GHF_E_FORMAT  (every item) one of the codes is not a complete prefix code
 * The words named by ghf_decode_images_batch_stats receive this call's rounds and passes too. */
int ghf_decode_bodies_batch_planes_shared(ghf_ctx* ctx, const uint8_t* const* d_stream_ptrs, const uint64_t* d_stream_bytes,
                                          const ghf_code* d_codes, uint32_t count, uint32_t elem_bytes,
                                          uint8_t* const* d_out_ptrs, const uint64_t* d_out_caps, uint64_t* d_out_bytes,
                                          int* d_item_status /* [count] */);

/* ---- the plane batch calls with raw planes ------------------------------------
 * No reference counterpart (include/compressor.h:62-73 always codes what it is given; 87-92 always decodes).  A mantissa
 * plane of normal floats holds nearly uniform bytes: its code has 7 to 10 bits, its bodies store MORE than the plane's
 * bytes (each rounds up behind an end mark) and the bodies-only decoder spends most of its passes on it.  The _forms calls
 * store such a plane RAW: slot j = i * E + p of a raw plane p holds the n_i bytes in[p], in[p + E], ... of item i and
 * nothing else -- no magic, no header, no end mark, as the raw form of ghf_compress_planes_forms.  A dense plane's slot stays
 * byte for byte what ghf_compress_batch_planes_shared writes, so ghf_write_header(d_codes + p) || body is still a
 * standalone .crs2.  Which planes are raw is ONE host value for the batch, uint32_t raw_planes (bit p = plane p), passed to
 * every call; no container records it.  A bit at or above elem_bytes: GHF_E_INVAL at call level.  raw_planes == 0 gives
 * exactly what the _shared call of the same name gives, in every output array.
 * Conventions, call-level errors and per-slot / per-item statuses are those of the calls above, with these rules:
 *   - d_codes[p] of a raw plane is never read: it may be garbage.  Only the codes of the dense planes are vetted; a bad one
 *     is GHF_E_FORMAT as in the _shared call (compress: on that plane's slots; decode: on every item, nothing written).
 *   - the order of the verdicts is the _shared call's: FORMAT, EMPTY / INVAL, CAP, CORRUPT.
 *   - nothing at or beyond d_out_caps is written; no byte outside stream[0 .. d_stream_bytes[j]) is read.
 *   - ghf_batch_seek_pack does not change: on the index of ghf_compress_batch_planes_forms it gives the records of the dense
 *     slots as ever; a raw slot's slice of the index was not written, so what the call reports for a raw slot (status,
 *     size, record bytes) is NOT SPECIFIED and the caller ignores it -- a raw slot has no record. */

/* No reference counterpart (include/compressor.h:62-73 never asks whether coding pays; 87-92).  One tiny launch, asynchronous,
 * never synchronises: *d_raw_planes (a device word) <- the mask of the planes that are better stored raw under d_codes
 * (device ghf_code[elem_bytes], 16-byte aligned) given the counts d_hists (device u64[elem_bytes][257], as
 * ghf_histogram_batch_planes leaves them).  Plane p is raw exactly when
 *     sum over s < 256 of d_hists[p][s] * d_codes[p].length[s]  >=  8 * sum over s < 256 of d_hists[p][s]
 * and the right-hand sum is not 0 -- 64-bit integer arithmetic on the arrays as given, slot 256 (the end mark) not
 * counted.  With exact counts a raw plane then never stores more than its bodies would.  A code whose min_len / max_len
 * fail the length bounds (1 <= min_len <= max_len <= 32) leaves its plane dense: ghf_compress_batch_planes_forms reports that
 * code.  A null context or pointer, an elem_bytes other than 2, 4 or 8, misaligned d_codes: GHF_E_INVAL. */
int ghf_batch_planes_raw_auto(ghf_ctx* ctx, const uint64_t* d_hists /* [elem_bytes][257] */, const ghf_code* d_codes /* [elem_bytes] */,
                              uint32_t elem_bytes, uint32_t* d_raw_planes);

/* No reference counterpart (generalises include/compressor.h:62-73; 87-92 is the way back).  ghf_compress_batch_planes_shared
 * with the planes of raw_planes stored raw.  Arguments and per-slot statuses are that call's.  For a raw slot j of item i
 * with n_i elements: d_out_ptrs[j][0 .. n_i) <- the plane's bytes, d_out_bytes[j] <- n_i; GHF_E_CAP when n_i >
 * d_out_caps[j], and then nothing is written; GHF_E_EMPTY, and GHF_E_INVAL for a null item, an oversized item, a size that
 * is not a multiple of elem_bytes or a null / misaligned slot pointer, as for a dense slot; never GHF_E_FORMAT or
 * GHF_E_NOCODE.  A raw slot's slice of `index` is not written.  ghf_compress_batch_planes_shared_bound (>= n_i) stays the
 * capacity that always suffices. */
int ghf_compress_batch_planes_forms(ghf_ctx* ctx, const uint8_t* const* d_in_ptrs, const uint64_t* d_in_bytes,
                                    size_t max_item_bytes, uint32_t count, uint32_t elem_bytes, const ghf_code* d_codes,
                                    uint32_t raw_planes, uint8_t* const* d_out_ptrs, const uint64_t* d_out_caps,
                                    uint64_t* d_out_bytes, const ghf_batch_index* index /* optional */,
                                    int* d_item_status /* [count * elem_bytes] */);

/* No reference counterpart (include/compressor.h:62-73 is the way there; generalises 87-92).  ghf_decode_batch_planes_shared
 * (the live side-car) with the planes of raw_planes stored raw.  A raw slot needs a non-null, 16-byte aligned pointer
 * (GHF_E_INVAL otherwise) and d_stream_bytes[j] == d_n_elems[i] (GHF_E_CORRUPT otherwise, seen before the item's first
 * store); its slice of `index` is not read. */
int ghf_decode_batch_planes_forms(ghf_ctx* ctx, const uint8_t* const* d_stream_ptrs, const uint64_t* d_stream_bytes,
                                  const ghf_code* d_codes, const ghf_batch_index* index, const uint64_t* d_n_elems,
                                  uint32_t count, uint32_t elem_bytes, uint32_t raw_planes, uint8_t* const* d_out_ptrs,
                                  const uint64_t* d_out_caps, uint64_t* d_out_bytes, int* d_item_status /* [count] */);

/* No reference counterpart (include/compressor.h:62-73 is the way there; generalises 87-92).
 * ghf_decode_bodies_batch_planes_shared (nothing but the bytes; d_out_ptrs == NULL: sizes only) with the planes of raw_planes
 * stored raw.  A raw slot's symbol count IS d_stream_bytes[j]: 0 or more than GHF_BATCH_MAX_ITEM / elem_bytes is
 * GHF_E_INVAL (as is a null or misaligned pointer).  A raw slot takes part in "the planes of one item hold the same number
 * of symbols" (GHF_E_CORRUPT), and an item whose planes are all raw decodes from the sizes alone.  The raw planes of an item
 * are held against their bounds, the cap (GHF_E_CAP) and each other before the item's first store. */
int ghf_decode_bodies_batch_planes_forms(ghf_ctx* ctx, const uint8_t* const* d_stream_ptrs, const uint64_t* d_stream_bytes,
                                         const ghf_code* d_codes, uint32_t count, uint32_t elem_bytes, uint32_t raw_planes,
                                         uint8_t* const* d_out_ptrs, const uint64_t* d_out_caps, uint64_t* d_out_bytes,
                                         int* d_item_status /* [count] */);

/* No reference counterpart (include/compressor.h:62-73 is the way there; generalises 87-92).
 * ghf_decode_bodies_batch_planes_shared_seek (bodies with their run records, below) with the planes of raw_planes stored raw.
 * A raw slot has no record: d_rec_ptrs[j] and d_rec_bytes[j] are ignored and may be null / 0 (the two arrays themselves are
 * required).  Its count is d_stream_bytes[j], under the bounds of ghf_decode_bodies_batch_planes_forms, and must agree with
 * the records of the dense planes (GHF_E_CORRUPT).  As there, all pointers, record headers and counts of an item are
 * vetted before its first store. */
int ghf_decode_bodies_batch_planes_forms_seek(ghf_ctx* ctx, const uint8_t* const* d_stream_ptrs /* [count * elem_bytes] */,
                                              const uint64_t* d_stream_bytes, const uint8_t* const* d_rec_ptrs /* [count * elem_bytes] */,
                                              const uint64_t* d_rec_bytes, const ghf_code* d_codes /* [elem_bytes] */, uint32_t count,
                                              uint32_t elem_bytes, uint32_t raw_planes, uint8_t* const* d_out_ptrs /* [count] */,
                                              const uint64_t* d_out_caps, uint64_t* d_out_bytes, int* d_item_status /* [count] */);

/* ---- stored shared-code bodies: the run record, the persistent form of a batch's side-car -------------
 * No reference counterpart (the reference compresses one file per process, include/compressor.h:62-73, and reads one back,
 * include/compressor.h:87-92).  ghf_decode_batch_shared and ghf_decode_batch_planes_shared need the live ghf_batch_index:
 * 6.25 % of the input in device memory, gone with the process that compressed.  The bodies-only calls need nothing but the
 * bytes and find every code boundary again, which codes of 7 to 10 bits (uniform bytes, mantissa planes) make slow.  A
 * RUN RECORD is what a stored body keeps beside it instead: ghf_batch_seek_pack writes one per body from the live
 * side-car, and the two _seek decoders read (body, record, the one code) in ONE launch, one workgroup per item, every
 * symbol decoded once.  No existing call and no .crs2 byte changes.
 *
 * A body is an item of ghf_compress_batch_shared, or slot i * elem_bytes + p of ghf_compress_batch_planes_shared.  Its
 * record, all fields little-endian:
 *     +0  u32 magic      "GBR1" (0x31524247)
 *     +4  u32 n_symbols  1 .. GHF_BATCH_MAX_ITEM: what the body decodes to
 *     +8  u16 run_bits[ceil(n_symbols / 128)]   the bits the codes of data symbols [128 r, 128 r + 128) take; the last
 *                                               run may be short; the end mark is not counted
 *         zero bytes up to a multiple of 8
 * 72 bytes for an item of 4 KiB (1.8 %), 1032 for one of 64 KiB (1.6 %).
 *
 * Conventions are those of the shared-code batch calls: every array is DEVICE memory; asynchronous on the context's
 * stream, never synchronises; failures are per slot or per item (GHF_OK is written as well; the size reported for a failed
 * one is 0) and never latch the context's status word; the context's caches are left alone; count == 0 queues nothing.
 * Call-level errors (returned at once, nothing queued, checked before anything touches HIP): a null context or array
 * (d_out_ptrs may be null, see below), an elem_bytes the call does not take, an index that does not cover count *
 * elem_bytes slots, d_out_ptrs without d_out_caps, a null or not 16-byte aligned code array: GHF_E_INVAL.  Stream and
 * record pointers are 16-byte aligned; decode outputs need no alignment.  Not supported: images of ghf_compress_batch
 * (a code per item), and the .crs format. */

/* No reference counterpart (include/compressor.h:62-73, 87-92).  Host only: 8 + 2 * ceil(n_symbols / 128), rounded up to
 * 8: the size of the record of a body of n_symbols. */
size_t ghf_batch_seek_bytes(size_t n_symbols);
/* No reference counterpart (include/compressor.h:62-73, 87-92).  Host only: ghf_batch_seek_bytes(max_item_bytes) rounded up
 * to 16, so that the slots of many records can be cut from one aligned buffer. */
size_t ghf_batch_seek_bound(size_t max_item_bytes);

/* No reference counterpart (include/compressor.h:62-73, 87-92).  The live side-car of a shared-code compress call -> one
 * record per body, in one launch.  elem_bytes 1: `index` is the one ghf_compress_batch_shared filled, body i has
 * d_in_bytes[i] symbols.  elem_bytes 2, 4, 8: the one ghf_compress_batch_planes_shared filled (count * elem_bytes slices),
 * slot i * elem_bytes + p has d_in_bytes[i] / elem_bytes symbols.  Slot j's record goes to d_rec_ptrs[j] (16-byte aligned),
 * d_rec_bytes[j] <- its size.  A refused slot writes nothing and reports 0 bytes.  d_slot_status[j] <-
 *   GHF_E_EMPTY   0 symbols
 *   GHF_E_INVAL   more symbols than a slice of the index covers; a size that is not a multiple of elem_bytes; a null or
 *                 misaligned record pointer
 *   GHF_E_CAP     the record is larger than d_rec_caps[j]
 *   GHF_E_CORRUPT the slice is not the side-car of a body: chunk_bit[0] != 0 (the images of ghf_compress_batch start behind
 *                 their header), a block that does not start where its predecessor's last segment ends, segment ends that
 *                 do not grow, a run of more than 65535 bits */
int ghf_batch_seek_pack(ghf_ctx* ctx, const ghf_batch_index* index, const uint64_t* d_in_bytes /* [count] */, uint32_t count,
                        uint32_t elem_bytes, uint8_t* const* d_rec_ptrs /* [count * elem_bytes] */,
                        const uint64_t* d_rec_caps, uint64_t* d_rec_bytes, int* d_slot_status /* [count * elem_bytes] */);

/* No reference counterpart (include/compressor.h:62-73 is the way there; generalises 87-92).  Item i = the body at
 * d_stream_ptrs[i] (d_stream_bytes[i] of it, which may exceed the body) and its record at d_rec_ptrs[i] (d_rec_bytes[i] of
 * it) -> d_out_ptrs[i][0 .. n_i), d_out_bytes[i] <- n_i, the record's n_symbols.  d_out_ptrs == NULL (then d_out_caps is
 * ignored): sizes only -- the pointers and each record's shape are checked, d_out_bytes[i] <- n_i, the stream is not read.
 * The code is vetted first, with the rules of ghf_decode_batch_shared: GHF_E_FORMAT on EVERY item, nothing written.  Then,
 * per item, nothing in a record is trusted.  d_item_status[i] <-
 *   GHF_E_INVAL   a null or misaligned stream or record pointer; a null output pointer in decode mode; d_stream_bytes[i]
 *                 greater than ghf_compress_batch_shared_bound(GHF_BATCH_MAX_ITEM)
 *   GHF_E_FORMAT  the record: wrong magic, n_symbols of 0 or above GHF_BATCH_MAX_ITEM, d_rec_bytes[i] !=
 *                 ghf_batch_seek_bytes(n_symbols)
 *   GHF_E_CAP     n_symbols > d_out_caps[i]; checked before any store
 *   GHF_E_CORRUPT a run starts or ends beyond bit 8 * d_stream_bytes[i]; a run does not land exactly on its recorded end;
 *                 a window starts no code; an end mark lies among the data; the end mark does not follow the last symbol
 *                 whole
 * No byte outside stream[0 .. d_stream_bytes[i]) or record[0 .. d_rec_bytes[i]) is read; nothing at or beyond d_out_caps[i]
 * is written (an item that fails with GHF_E_CORRUPT may have written in front of it). */
int ghf_decode_bodies_batch_shared_seek(ghf_ctx* ctx, const uint8_t* const* d_stream_ptrs, const uint64_t* d_stream_bytes,
                                        const uint8_t* const* d_rec_ptrs, const uint64_t* d_rec_bytes, const ghf_code* d_code,
                                        uint32_t count, uint8_t* const* d_out_ptrs, const uint64_t* d_out_caps,
                                        uint64_t* d_out_bytes, int* d_item_status /* [count] */);

/* No reference counterpart (include/compressor.h:62-73 is the way there; generalises 87-92).  The same for the slots of
 * ghf_compress_batch_planes_shared: d_stream_ptrs / d_stream_bytes / d_rec_ptrs / d_rec_bytes are [count * elem_bytes],
 * d_codes is [elem_bytes]; output and status are PER ITEM and written as in ghf_decode_batch_planes_shared, d_out_bytes[i]
 * <- n_i * elem_bytes, d_out_caps[i] is in bytes.  All elem_bytes codes (GHF_E_FORMAT on every item) and all elem_bytes
 * pointers and record headers of an item are vetted before its first store.  Status as above, for any plane of the item,
 * and GHF_E_CORRUPT when the records of one item disagree on n_symbols; GHF_E_CAP: n_symbols * elem_bytes > d_out_caps[i]. */
int ghf_decode_bodies_batch_planes_shared_seek(ghf_ctx* ctx, const uint8_t* const* d_stream_ptrs /* [count * elem_bytes] */,
                                               const uint64_t* d_stream_bytes, const uint8_t* const* d_rec_ptrs /* [count * elem_bytes] */,
                                               const uint64_t* d_rec_bytes, const ghf_code* d_codes /* [elem_bytes] */, uint32_t count,
                                               uint32_t elem_bytes, uint8_t* const* d_out_ptrs /* [count] */,
                                               const uint64_t* d_out_caps, uint64_t* d_out_bytes, int* d_item_status /* [count] */);

/* ---- byte planes: an element range ---------------------------------------------
 * No reference counterpart (generalises the flat output of include/compressor.h:87-92).  ghf_planes_merge for elements
 * [first, first + count) of the planes: d_out[0 .. count * elem_bytes) receives them and nothing else is written.
 * d_planes, plane_stride and d_out are 16-byte aligned as for ghf_planes_merge; first is arbitrary.  Only bytes
 * [first & ~15, (first + count + 15) & ~15) of a plane are read, and these must lie inside plane_stride.  Asynchronous on
 * the stream; does not look at the context's status word.  Checked before anything touches HIP: a null context or pointer,
 * another elem_bytes, misalignment, first + count or count * elem_bytes beyond size_t: GHF_E_INVAL; then count == 0:
 * GHF_E_EMPTY; then plane_stride < first + count: GHF_E_CAP.  One streaming kernel of ghf_planes_merge's shape; a first that
 * is no multiple of 16 costs a second aligned 16-byte load per plane vector and a byte funnel in registers. */
int ghf_planes_merge_range(ghf_ctx* ctx, const uint8_t* d_planes, size_t plane_stride, size_t first, size_t count,
                           uint32_t elem_bytes, uint8_t* d_out);

/* No reference counterpart: Decompressor::decompress(), include/compressor.h:87-92, for a part of a typed tensor.
 * d_out[0 .. count * elem_bytes) receives elements [first, first + count) of what the elem_bytes plane images decode to:
 * every plane is decoded from the start of the 4096-symbol block that holds `first` into the context's workspace (as
 * ghf_decode_range does it; from tables one launch expands the covered blocks of all planes), then ghf_planes_merge_range
 * takes the part asked for.  Asynchronous on the stream, never synchronises.  h_stream_ptrs / h_stream_bytes / d_codes
 * are those of ghf_decode_planes (HOST arrays of elem_bytes entries, d_codes on the device).  Exactly one source of
 * block starts is given, the other is NULL:
 *   indexes                                  elem_bytes live side-cars (a HOST array);
 *   (h_infos, h_table_ptrs, h_table_bytes)   elem_bytes parsed seek tables (HOST arrays); the table images are DEVICE
 *                                            memory, 16-byte aligned.  Only the covered blocks are expanded.
 * n_elems is what the side-cars or tables say; all of them must agree.  A stream that has neither is not served here: index
 * it once with ghf_decoded_size + ghf_seek_pack(index = NULL) and keep the table.
 * Checked in this order, all before anything is queued: a null context or required pointer, another elem_bytes, both
 * sources or neither, a stream / table / output pointer that is null or misaligned, a malformed index, planes that disagree
 * on n_symbols, first + count > n_elems, count * elem_bytes beyond size_t: GHF_E_INVAL; a table whose table_bytes is not what
 * its header implies (any plane): GHF_E_FORMAT; cap < count * elem_bytes: GHF_E_CAP; count == 0: GHF_OK, nothing queued (the
 * rule of ghf_decode_range).
 * As in ghf_decode_planes the merge stores nothing when a decode before it latched GHF_E_CORRUPT or GHF_E_FORMAT; ghf_sync
 * reports the status.  From side-cars the context's caches are left as ghf_decode_range leaves them (the tables of
 * ghf_decode_prepare are forgotten); from seek tables the call builds its tables in a buffer of its own and does not touch
 * the prepared tables. */
int ghf_decode_planes_range(ghf_ctx* ctx, const uint8_t* const* h_stream_ptrs, const size_t* h_stream_bytes,
                            const ghf_code* d_codes, const ghf_index* indexes, const ghf_seek_info* h_infos,
                            const uint8_t* const* h_table_ptrs, const size_t* h_table_bytes, uint32_t elem_bytes,
                            uint64_t first, uint64_t count, uint8_t* d_out, size_t cap);

/* ---- byte planes against a base tensor: XOR-delta compress, decode, range -----
 * Callers that hold a SERIES of tensors -- successive checkpoints, a fine-tuned model beside its base, optimizer state
 * step after step -- compress `new ^ base` instead of `new`: the sign / exponent byte and the top mantissa bits of an
 * element rarely change, so the high planes of the XOR are almost all zeros.  XOR is lossless for every bit pattern and
 * its own inverse.  These calls are the byte-plane calls above with the XOR inside the streaming kernels that touch every
 * interleaved vector anyway: nothing is materialised, and the .crs2 format does not change -- EVERY PLANE IS AN ORDINARY
 * STANDALONE .crs2 IMAGE, of the bytes of d_in ^ d_base, which the reference, ghf_decode, the seek table and the range
 * calls read.
 *
 * d_base is device memory, 16-byte aligned, and holds the same n_elems * elem_bytes bytes as d_in / d_out (for the two
 * range calls: count * elem_bytes bytes, see there); nothing outside them is read.  Conventions, argument checks, the
 * order of the checks and the error codes of every call are those of the plain call it mirrors; in addition a null d_base
 * is refused where the other null pointers are and a misaligned one where the other misaligned pointers are: GHF_E_INVAL,
 * nothing queued, checked before anything touches HIP.
 * In the merging calls (ghf_planes_merge_delta, ghf_planes_merge_range_delta, ghf_decode_planes_delta,
 * ghf_decode_planes_range_delta) d_base == d_out is allowed, "XOR the delta into the base": every lane reads the base
 * vector it then overwrites.  ANY OTHER OVERLAP of d_base with d_out, and any overlap of either with the planes, is
 * undefined. */

/* No reference counterpart (generalises the flat count of include/encoder.h:123-150, which include/compressor.h:62-73
 * runs once per file).  ghf_histogram_planes of d_in ^ d_base in one pass over both buffers: d_hists (device
 * u64[elem_bytes][257]) feeds ghf_build_codes and ghf_planes_image_bytes unchanged, so "delta or plain, which is smaller?"
 * costs two histogram passes. */
int ghf_histogram_planes_delta(ghf_ctx* ctx, const uint8_t* d_in, const uint8_t* d_base, size_t n_elems, uint32_t elem_bytes,
                               unsigned flags, uint64_t* d_hists /* [elem_bytes][257] */);

/* No reference counterpart (generalises the flat input of include/compressor.h:62-73).  ghf_planes_split of d_in ^ d_base:
 * byte b of element k of the XOR goes to d_planes[b * plane_stride + k]. */
int ghf_planes_split_delta(ghf_ctx* ctx, const uint8_t* d_in, const uint8_t* d_base, size_t n_elems, uint32_t elem_bytes,
                           uint8_t* d_planes, size_t plane_stride);

/* No reference counterpart (generalises the flat output of include/compressor.h:87-92).  The inverse of
 * ghf_planes_split_delta: d_out[0 .. n_elems * elem_bytes) <- ghf_planes_merge of the planes, XOR d_base.  d_base == d_out
 * is allowed.  Does not look at the context's status word. */
int ghf_planes_merge_delta(ghf_ctx* ctx, const uint8_t* d_planes, size_t plane_stride, const uint8_t* d_base, size_t n_elems,
                           uint32_t elem_bytes, uint8_t* d_out);

/* No reference counterpart (generalises the flat output of include/compressor.h:87-92).  ghf_planes_merge_range with the
 * XOR: d_base[0 .. count * elem_bytes) holds base elements [first, first + count) -- the caller's shard or rows of the base,
 * 16-byte aligned and indexed exactly like d_out, whatever `first` is.  d_base == d_out is allowed. */
int ghf_planes_merge_range_delta(ghf_ctx* ctx, const uint8_t* d_planes, size_t plane_stride, const uint8_t* d_base, size_t first,
                                 size_t count, uint32_t elem_bytes, uint8_t* d_out);

/* No reference counterpart: Compressor::compress(), include/compressor.h:62-73, once per byte plane of d_in ^ d_base, its
 * count (include/encoder.h:123-150) made in one pass.  ghf_compress_planes_coded of d_in ^ d_base: the same flags
 * (GHF_PLANES_BUILD_CODES or the caller's d_codes), the same vetting, the same latching of GHF_E_FORMAT / GHF_E_NOCODE
 * (d_out_bytes UNSPECIFIED behind a latched status).  On the stream: ghf_histogram_planes_delta into counters of the
 * context; the codes; ghf_planes_split_delta into the workspace; per plane the unchanged ghf_encode_plan and
 * ghf_encode_emit.  Every image, size, code and side-car is byte for byte what ghf_compress_planes_coded writes for a
 * buffer that holds d_in ^ d_base; the context's caches are forgotten as there. */
int ghf_compress_planes_delta(ghf_ctx* ctx, const uint8_t* d_in, const uint8_t* d_base, size_t n_elems, uint32_t elem_bytes,
                              ghf_code* d_codes /* [elem_bytes] 16-byte aligned: in or out with BUILD_CODES */, unsigned flags,
                              uint8_t* d_out, size_t slot_bytes, uint64_t* d_out_bytes, const ghf_index* indexes);

/* No reference counterpart: Decompressor::decompress(), include/compressor.h:87-92, once per byte plane.
 * ghf_decode_planes with ghf_planes_merge_delta last: d_out <- what the images decode to, XOR d_base.  indexes == NULL
 * SYNCHRONISES as it does there.  d_base == d_out is allowed.  Behind a latched status the merge stores nothing: in place,
 * d_out then still holds the base. */
int ghf_decode_planes_delta(ghf_ctx* ctx, const uint8_t* const* h_stream_ptrs, const size_t* h_stream_bytes,
                            const ghf_code* d_codes, const ghf_index* indexes, const uint8_t* d_base, size_t n_elems,
                            uint32_t elem_bytes, uint8_t* d_out, size_t cap, uint64_t* d_out_bytes);

/* No reference counterpart: Decompressor::decompress(), include/compressor.h:87-92, for a part of a typed tensor.
 * ghf_decode_planes_range with ghf_planes_merge_range_delta last, from live side-cars or from seek tables: d_base[0 ..
 * count * elem_bytes) holds base elements [first, first + count), as for ghf_planes_merge_range_delta; d_base == d_out is
 * allowed.  count == 0: GHF_OK, nothing queued. */
int ghf_decode_planes_range_delta(ghf_ctx* ctx, const uint8_t* const* h_stream_ptrs, const size_t* h_stream_bytes,
                                  const ghf_code* d_codes, const ghf_index* indexes, const ghf_seek_info* h_infos,
                                  const uint8_t* const* h_table_ptrs, const size_t* h_table_bytes, const uint8_t* d_base,
                                  uint32_t elem_bytes, uint64_t first, uint64_t count, uint8_t* d_out, size_t cap);

/* Multi-GPU decode of a stream that has no side-car ("per-rank self-sync + one all-gather of symbol
 * counts"; the reference's decoders, canonical_huff_encoder.cc:377-568, are single-stream).  The caller cuts the body
 * at byte positions; a rank's piece is its own bytes followed by >= 8 bytes of look-ahead from the next piece (zeros
 * behind the stream's end).  d_piece / piece_bytes: the piece with its look-ahead; first_bit (< 512): where the first
 * code boundary of the piece is assumed to be; end_bit = 8 * (own bytes): codes that start at or behind it belong to
 * the next piece.  Out (host, the call synchronises): landing = how many bits the last code (or the one in progress)
 * runs past end_bit, i.e. the NEXT piece's first_bit; n_symbols = codes that start in [first_bit, end_bit), up to the
 * end mark if the piece holds it (has_end_mark).  Because Huffman codes self-synchronise, a wrong first_bit only
 * spoils the first few symbols; iterate first_bit[g+1] = landing[g] until nothing changes (sharded.py does), then
 * ghf_decode(d_piece, piece_bytes, d_code, index = NULL, ...) decodes the piece with the side-car this call rebuilt. */
int ghf_sync_piece(ghf_ctx* ctx, const uint8_t* d_piece, size_t piece_bytes, uint32_t first_bit, uint64_t end_bit,
                   const ghf_code* d_code, uint64_t* landing, uint64_t* n_symbols, int* has_end_mark);

/* ---- byte planes in three forms: raw planes beside dense and sparse ones -------------
 * The mantissa planes of a float tensor gain nothing from a Huffman code: their images are LARGER than the planes, and
 * every one of them costs a whole compress pass and a whole decode pass on 8-bit codes.  THE RAW FORM of a plane is the
 * plane's n_elems bytes at the start of its slot and nothing else (no container, no magic, no header): d_out_bytes[p] =
 * n_elems, the slot's code is unwritten and its side-car entry zeroed.  It is the third form beside the dense one (a
 * standalone .crs2 image) and the sparse one; the calls of this section take any mix of the three.
 * No .crs2, seek-table, run-record or rank-table byte changes, and a decode is told which planes are raw as it is told
 * which are sparse.
 *
 * A raw plane is never copied: the split writes it straight into the caller's slot and the merge reads it there, through
 * kernels that take ONE ADDRESS PER PLANE (k_planes_split_to, k_planes_merge_from, k_planes_merge_range_from).
 * IN THIS FAMILY d_base IS OPTIONAL: NULL is the plain call, non-NULL XORs the interleaved side against it as the calls
 * of DESIGN.md section 19 do; a misaligned d_base is still GHF_E_INVAL.  Every device pointer is 16-byte aligned.
 * Call-level refusals come before anything touches HIP, with nothing queued, in the order of the sparse calls; in
 * addition a raw_planes with a bit at or above elem_bytes, GHF_RAW_AUTO together with an explicit bit, GHF_RAW_AUTO in a
 * decode, a plane named in both explicit masks, a raw stream whose size is not n_elems: GHF_E_INVAL. */
#define GHF_RAW_AUTO 0x80000000u
struct ghf_sparse_rank_info; /* the parsed rank table of a sparse plane: defined with the rank tables below */

/* No reference counterpart (generalises the flat input of include/compressor.h:62-73).  ghf_planes_split with a
 * destination per plane: byte p of element k of d_in -- of d_in ^ d_base when d_base is not NULL -- goes to
 * h_plane_ptrs[p][k].  h_plane_ptrs is a HOST array of elem_bytes DEVICE pointers, each 16-byte aligned and good for
 * n_elems bytes, read before the call returns; the planes may lie anywhere and in any order but must not overlap.
 * Asynchronous, never synchronises. */
int ghf_planes_split_to(ghf_ctx* ctx, const uint8_t* d_in, const uint8_t* d_base /* optional */, size_t n_elems,
                        uint32_t elem_bytes, uint8_t* const* h_plane_ptrs /* HOST [elem_bytes] */);

/* No reference counterpart (generalises the flat output of include/compressor.h:87-92).  The inverse: d_out[0 .. n_elems
 * * elem_bytes) <- the planes at h_plane_ptrs (HOST [elem_bytes], each 16-byte aligned), XOR d_base when it is not NULL.
 * d_base == d_out is allowed.  Does not look at the context's status word. */
int ghf_planes_merge_from(ghf_ctx* ctx, const uint8_t* const* h_plane_ptrs /* HOST [elem_bytes] */,
                          const uint8_t* d_base /* optional */, size_t n_elems, uint32_t elem_bytes, uint8_t* d_out);

/* No reference counterpart (generalises the flat output of include/compressor.h:87-92).  ghf_planes_merge_range with a
 * source per plane: h_plane_ptrs[p] is the address of plane p's byte of the run's FIRST element, d_out[0 .. count *
 * elem_bytes) receives the run.  The addresses need not be aligned but all have the same remainder modulo 16 (GHF_E_INVAL
 * otherwise) -- what holds when every plane begins 16-byte aligned at element 0 or at a block of 4096 elements.  Nothing
 * is read outside the aligned 16-byte vectors that hold the run's bytes.  d_base (optional) holds the base elements of
 * the run itself at d_base[0 .. count * elem_bytes), unskewed and indexed like d_out; d_base == d_out is allowed. */
int ghf_planes_merge_range_from(ghf_ctx* ctx, const uint8_t* const* h_plane_ptrs /* HOST [elem_bytes] */,
                                const uint8_t* d_base /* optional */, size_t count, uint32_t elem_bytes, uint8_t* d_out);

/* No reference counterpart: Compressor::compress(), include/compressor.h:62-73, once per stored stream that has a code,
 * and not at all for a raw plane.  The slots, sizes, codes, side-cars and rank tables are laid out as by
 * ghf_compress_planes_sparse_ranked: 2 * elem_bytes slots of slot_bytes >= ghf_planes_slot_bytes of n_elems.  A dense
 * plane's image, size, code and side-car are byte for byte what ghf_compress_planes writes, a sparse plane's what the
 * sparse call writes; a raw plane is written by the split itself, straight into slot p: no workspace copy, no histogram
 * pass of its own, no code build, no packing, and no byte of the slot behind n_elems is written.  d_ranks == NULL: no
 * rank tables.
 * raw_planes / sparse_planes: explicit bits below elem_bytes (a plane named in both: GHF_E_INVAL), or GHF_RAW_AUTO /
 * GHF_SPARSE_AUTO.  With GHF_RAW_AUTO a plane that is not sparse is raw EXACTLY when the image it would get is at least
 * n_elems bytes -- the size ghf_planes_image_bytes gives under the code ghf_build_codes builds from its counts -- so no
 * such plane stores more than n_elems bytes.  With GHF_SPARSE_AUTO the rule of the sparse call (at least n_elems -
 * n_elems / 4 zero bytes) picks the sparse planes first; with BOTH masks automatic only when n_elems > 2 *
 * ghf_header_bytes(1): a sparse plane stores two headers, and at or below that size raw is always the smaller.
 * *h_raw_planes, *h_sparse_planes and h_n_vals (HOST) report what was chosen and are what the decode must be told.
 * The call SYNCHRONISES with the host AT MOST ONCE: ghf_histogram_planes, and with GHF_RAW_AUTO ghf_build_codes for all
 * planes and ghf_planes_image_bytes, are queued, and one copy brings back the counts and the sizes; the dense planes are
 * packed with those codes, there is no second build.  With both masks explicit and sparse_planes == 0 the call NEVER
 * synchronises, and h_n_vals is zeroed.  With every plane raw the call is one split launch and the size stores.
 * Device failures latch as for ghf_compress_planes_coded. */
int ghf_compress_planes_forms(ghf_ctx* ctx, const uint8_t* d_in, const uint8_t* d_base /* optional */, size_t n_elems,
                              uint32_t elem_bytes, unsigned raw_planes, unsigned sparse_planes, uint8_t* d_out, size_t slot_bytes,
                              uint64_t* d_out_bytes /* [2 * elem_bytes] */, ghf_code* d_codes /* [2 * elem_bytes] optional OUT */,
                              ghf_index* h_indexes /* [2 * elem_bytes] optional OUT */, uint8_t* d_ranks /* optional */,
                              size_t rank_slot_bytes, unsigned* h_raw_planes /* OUT */, unsigned* h_sparse_planes /* OUT */,
                              size_t* h_n_vals /* [elem_bytes] OUT */);

/* No reference counterpart: Decompressor::decompress(), include/compressor.h:87-92, once per stored stream that has a
 * code.  ghf_decode_planes_sparse with raw planes: raw_planes, sparse_planes and h_n_vals are what the compress call
 * reported.  For a raw plane h_stream_ptrs[p] (16-byte aligned) holds the plane itself and h_stream_bytes[p] is n_elems,
 * GHF_E_INVAL otherwise with nothing queued; its code and index entries are ignored.  The plane is never copied: the
 * merge, which comes last and stores nothing behind a latched status, reads it where it lies.  d_base == d_out is
 * allowed, and behind a latched status d_out then still holds the base.  With every plane raw the call is one merge
 * launch and d_codes may be NULL.  indexes == NULL SYNCHRONISES per stream that has a code, as ghf_decode_planes does. */
int ghf_decode_planes_forms(ghf_ctx* ctx, const uint8_t* const* h_stream_ptrs /* [2 * elem_bytes] */,
                            const size_t* h_stream_bytes /* [2 * elem_bytes] */, const ghf_code* d_codes /* [2 * elem_bytes] */,
                            const ghf_index* indexes /* [2 * elem_bytes] or NULL */, const uint8_t* d_base /* optional */,
                            unsigned raw_planes, unsigned sparse_planes, const size_t* h_n_vals /* [elem_bytes] */, size_t n_elems,
                            uint32_t elem_bytes, uint8_t* d_out, size_t cap, uint64_t* d_out_bytes);

/* No reference counterpart: Decompressor::decompress(), include/compressor.h:87-92, for a part of a typed tensor stored
 * in any mix of the three forms.  ghf_decode_planes_sparse_range with raw planes, from side-cars or from seek tables;
 * never synchronises.  Nothing is decoded or expanded for a raw plane: its index, seek info, table and code entries are
 * not read (they may be NULL or zero), its size is n_elems (GHF_E_INVAL otherwise) and its source is h_stream_ptrs[p] +
 * first.  With raw planes and no sparse one the other planes are decoded from the seek block that holds `first`, as
 * ghf_decode_planes_range does it; with a sparse plane from the rank block, by the plan of the sparse range call.  The
 * refusals and their order are that call's; count == 0: GHF_OK, nothing queued. */
int ghf_decode_planes_forms_range(ghf_ctx* ctx, const uint8_t* const* h_stream_ptrs /* [2 * elem_bytes] */,
                                  const size_t* h_stream_bytes /* [2 * elem_bytes] */, const ghf_code* d_codes /* [2 * elem_bytes] */,
                                  const ghf_index* indexes /* [2 * elem_bytes] or NULL */,
                                  const ghf_seek_info* h_infos /* [2 * elem_bytes] or NULL */,
                                  const uint8_t* const* h_table_ptrs /* [2 * elem_bytes] or NULL */,
                                  const size_t* h_table_bytes /* [2 * elem_bytes] or NULL */,
                                  const struct ghf_sparse_rank_info* h_rank_infos /* [elem_bytes] */,
                                  const uint8_t* const* h_rank_ptrs /* [elem_bytes] */, const uint8_t* d_base /* optional */,
                                  unsigned raw_planes, unsigned sparse_planes, size_t n_elems, uint32_t elem_bytes, uint64_t first,
                                  uint64_t count, uint8_t* d_out, size_t cap);

/* ---- byte planes: many rows in one call ------------------------------------------
 * The range calls above serve one range per call and every range is a host argument; a lookup of rows of an embedding
 * table that stays compressed in device memory has its row indices on the device and wants them all in one launch. */
#define GHF_GATHER_MAX_ROW_ELEMS 32768u /* the longest row of ghf_decode_planes_gather */

/* No reference counterpart: Decompressor::decompress(), include/compressor.h:87-92, for MANY parts of a typed tensor at
 * once.  ROW r is elements [d_index[r] *
 * index_stride, + row_elems) of the tensor, and its row_elems * elem_bytes interleaved bytes go to d_out + r * out_stride:
 * index_stride = row_elems is a lookup by row id, index_stride = 1 takes arbitrary element offsets; rows may repeat,
 * overlap in the source and come in any order.  The row indices are DEVICE memory, and the call queues ONE launch whatever
 * n_rows is (one workgroup per row); it never waits for the device.
 * The tensor is stored as ghf_compress_planes_forms stores it with sparse_planes == 0: plane p is a standalone .crs2 image
 * with a seek table from ghf_seek_pack, or raw (bit p of raw_planes).  The arrays are the first elem_bytes entries of the
 * forms calls' arrays; seek tables are the only source of run starts (a caller with live side-cars packs them once).
 * READ: the row indices; of a raw plane the rows' bytes where they lie; of a dense plane its code, the records of the
 * blocks a row covers and the stream bytes of the runs of 512 symbols it touches -- at most 511 symbols are decoded in
 * front of a row and 511 behind it.  WRITTEN: d_row_status[0 .. n_rows), and bytes [r * out_stride, r * out_stride +
 * row_elems * elem_bytes) of d_out for every row whose status is GHF_OK.  Nothing else: out_stride need not be a multiple
 * of 16, and padding between rows keeps what it held.
 * CALL-LEVEL REFUSALS come before anything touches HIP, queue nothing and leave the context's status alone, in this
 * order: a null context; elem_bytes not 2, 4 or 8; a raw_planes bit at or above elem_bytes; row_elems == 0 or above
 * GHF_GATHER_MAX_ROW_ELEMS; out_stride < row_elems * elem_bytes; a null pointer, a stream, table, d_codes or d_out that is
 * not 16-byte aligned, a d_index that is not 8-byte or a d_row_status that is not 4-byte aligned (d_codes, h_infos,
 * h_table_ptrs and h_table_bytes may be NULL when every plane is raw); a raw stream whose size is not n_elems; a dense
 * plane whose table says n_symbols != n_elems: GHF_E_INVAL; a dense plane's table whose table_bytes is not what its header
 * implies: GHF_E_FORMAT.  Then n_rows == 0: GHF_OK, nothing queued.
 * FAILURES ARE PER ROW: they land in d_row_status[r] and never latch the context.  A failed row stores NOTHING -- every
 * verdict of a row is reached before its first store -- and the other rows are unaffected.
 *   GHF_OK
 *   GHF_E_FORMAT  on every row: the code of a dense plane is not a complete prefix code of lengths <= 32
 *   GHF_E_INVAL   d_index[r] * index_stride overflows 64 bits, or the row passes n_elems
 *   GHF_E_CORRUPT for any dense plane: a covered block's start_bit + the sum of its run_bits lies beyond bit 8 *
 *                 stream_bytes, or is not the next block's start_bit; a covered run does not land exactly on its recorded
 *                 end, meets an end mark, or meets bits that start no code
 * The tables and streams come from disk and nothing in them is trusted: no byte outside stream[0 .. stream_bytes) or
 * outside a table is read, whatever they hold.  Start bits are 64-bit: planes of more than 2^32 stream bits are served. */
int ghf_decode_planes_gather(ghf_ctx* ctx, const uint8_t* const* h_stream_ptrs /* HOST [elem_bytes] device pointers 16-byte aligned */,
                             const size_t* h_stream_bytes /* [elem_bytes] */,
                             const ghf_code* d_codes /* DEVICE [elem_bytes] -- a raw plane's entry is never read */,
                             const ghf_seek_info* h_infos /* [elem_bytes] -- a raw plane's entry is not read */,
                             const uint8_t* const* h_table_ptrs /* [elem_bytes] seek-table images in device memory */,
                             const size_t* h_table_bytes /* [elem_bytes] */, unsigned raw_planes, size_t n_elems, uint32_t elem_bytes,
                             const uint64_t* d_index /* DEVICE [n_rows] */, uint64_t index_stride, uint32_t row_elems, uint32_t n_rows,
                             uint8_t* d_out, size_t out_stride /* bytes from one output row to the next */,
                             int32_t* d_row_status /* DEVICE [n_rows] */);

/* ---- byte planes: many rows of a tensor stored sparse or against a base -----------
 * ghf_decode_planes_gather serves a tensor of dense and raw planes that was compressed by itself; the forms that compress
 * best -- against a base tensor, and sparse planes on top of that -- are served here, with the same row rule. */
#define GHF_GATHER_SPARSE_MAX_ROW_ELEMS 8192u /* the longest row of ghf_decode_planes_gather_forms when a plane is sparse */

/* No reference counterpart: Decompressor::decompress(), include/compressor.h:87-92, for MANY parts of a typed tensor
 * stored in any mix of the three forms, against a base tensor where there is one.  The ROW RULE, the output rule and the
 * per-row statuses are those of ghf_decode_planes_gather: row r is elements [d_index[r] * index_stride, + row_elems), its
 * bytes go to d_out + r * out_stride at any alignment, rows may repeat, overlap and come in any order; ONE launch whatever
 * n_rows is, never a wait for the device, and nothing latches the context.
 * SLOTS are indexed as ghf_compress_planes_forms lays them out: slot j < elem_bytes holds plane j when it is dense or raw,
 * or its mask when it is sparse; slot elem_bytes + p the values of sparse plane p, ignored (pointers, sizes, code, info
 * and table) when h_rank_infos[p].n_vals == 0, as are the upper slots of every other plane.  Every stored stream that has
 * a code comes with its seek table from ghf_seek_pack (device memory, 16-byte aligned).  Every sparse plane comes with
 * its rank table (ghf_sparse_rank_pack, or d_ranks of the compress call) AS AN IMAGE IN DEVICE MEMORY: h_rank_ptrs is a
 * HOST array of DEVICE pointers, 8-byte aligned, h_rank_bytes[p] == ghf_sparse_rank_bytes of n_elems, and h_rank_infos[p]
 * is what ghf_sparse_rank_parse gave for it -- the range calls take the table on the host; this call reads cum[] per row
 * on the device.  With sparse_planes == 0 the three rank arrays may be NULL.
 * BASE: with d_base != NULL row r is the planes' bytes XOR d_base[first * elem_bytes .. + row_elems * elem_bytes), first
 * = d_index[r] * index_stride: d_base is the WHOLE base tensor, n_elems * elem_bytes bytes.  It is read byte by byte: no
 * alignment is required of it and none is refused.  d_base and d_out must not overlap: a gather is not in place.
 * ROW CAP: GHF_GATHER_MAX_ROW_ELEMS when sparse_planes == 0, GHF_GATHER_SPARSE_MAX_ROW_ELEMS otherwise: a row then
 * touches at most two rank blocks, 11 runs of a mask stream and 17 of a values stream.
 * READ: what ghf_decode_planes_gather reads of raw and dense planes; of a sparse plane two or three entries of cum[], the
 * records and stream bytes of the mask's runs of 512 bytes from the start of the row's rank block to the row's end, and of
 * the values' runs that hold the row's values; of the base the rows' bytes.  WRITTEN: d_row_status[0 .. n_rows), and
 * bytes [r * out_stride, r * out_stride + row_elems * elem_bytes) of d_out for every row whose status is GHF_OK.
 * CALL-LEVEL REFUSALS come before anything touches HIP, queue nothing and leave the context's status alone, in this
 * order: those of ghf_decode_planes_gather in its order (the row cap as above; the slots looked at are those of dense,
 * raw and sparse planes' own streams, a "dense stream" check applying to dense planes only); then a plane named in both
 * masks, GHF_RAW_AUTO or GHF_SPARSE_AUTO, or a sparse_planes bit at or above elem_bytes; then, with a sparse plane, a
 * null rank array, a null or misaligned rank pointer or an h_rank_bytes that is not ghf_sparse_rank_bytes of n_elems; then
 * a rank info whose n is not n_elems; then a mask table whose n_symbols is not ghf_sparse_mask_bytes of n_elems; then, for
 * a sparse plane with values, a null or misaligned values stream or table, or a values table whose n_symbols is not the
 * rank info's n_vals: all GHF_E_INVAL; a rank info whose other fields are not what ghf_sparse_rank_parse fills in, or a
 * seek table whose size contradicts its header: GHF_E_FORMAT.  Then n_rows == 0: GHF_OK, nothing queued.
 * FAILURES ARE PER ROW, as in ghf_decode_planes_gather; a failed row stores NOTHING: every verdict of a row, of all its
 * planes, is reached before its first store.
 *   GHF_OK
 *   GHF_E_FORMAT  on every row: the code of a stored stream is not a complete prefix code of lengths <= 32
 *   GHF_E_INVAL   d_index[r] * index_stride overflows 64 bits, or the row passes n_elems
 *   GHF_E_CORRUPT a dense plane, a mask stream or a values stream fails a block or run check of ghf_decode_planes_gather;
 *                 or for a sparse plane, with b0 = first / 32768: cum[b0], cum[b0 + 1] (and cum[b0 + 2] where the row
 *                 crosses into the next rank block) are not ordered, exceed n_vals, or step by more than the elements
 *                 of their block; the decoded mask holds a rank block to its end (or the tensor's) and the block's set
 *                 bits do not number the difference of its two entries; the row touches the last mask byte and a pad
 *                 bit is set; cum[b0] + the set bits in front of the row + the row's own exceed n_vals
 * As in DESIGN.md section 21 the mask is held against DIFFERENCES of rank entries, and only where a whole block is
 * decoded: a table whose entries were all shifted, or a wrong entry in front of a row that ends more than 4096 elements
 * before its block does, is not noticed and moves the row's values.  The rank table is as trusted as the streams' order
 * of bytes; what IS guaranteed whatever the tables and streams hold: no byte outside a stream, a seek table or a rank
 * table is read, and no byte outside the rows is written.
 * IDENTITY: with sparse_planes == 0 and d_base == NULL the output and the statuses are byte for byte those of
 * ghf_decode_planes_gather on the first elem_bytes entries of the arrays. */
int ghf_decode_planes_gather_forms(ghf_ctx* ctx, const uint8_t* const* h_stream_ptrs /* HOST [2 * elem_bytes] device pointers */,
                                   const size_t* h_stream_bytes /* [2 * elem_bytes] */, const ghf_code* d_codes /* DEVICE [2 * elem_bytes] */,
                                   const ghf_seek_info* h_infos /* [2 * elem_bytes] */,
                                   const uint8_t* const* h_table_ptrs /* [2 * elem_bytes] seek tables, device */,
                                   const size_t* h_table_bytes /* [2 * elem_bytes] */,
                                   const struct ghf_sparse_rank_info* h_rank_infos /* [elem_bytes] */,
                                   const uint8_t* const* h_rank_ptrs /* HOST [elem_bytes] DEVICE images */,
                                   const size_t* h_rank_bytes /* [elem_bytes] */,
                                   const uint8_t* d_base /* optional: the whole base tensor, n_elems * elem_bytes bytes */,
                                   unsigned raw_planes, unsigned sparse_planes, size_t n_elems, uint32_t elem_bytes,
                                   const uint64_t* d_index /* DEVICE [n_rows] */, uint64_t index_stride, uint32_t row_elems, uint32_t n_rows,
                                   uint8_t* d_out, size_t out_stride, int32_t* d_row_status /* DEVICE [n_rows] */);

/* ------------------------------------------------------------------------------------------------
 * one stream sharded over the GPUs of a node, one process (or thread) and one ghf_ctx per GPU,
 * RCCL over xGMI underneath.  The reference has no counterpart (it is single-threaded, single-stream:
 * include/compressor.h:62-73); what makes the shards ONE .crs2 stream, bit-exact with the single-stream
 * reference, is a single global code, which costs exactly two latency-bound exchanges:
 *   all-reduce(sum) of the 256 byte counts   (the end-mark slot [256] stays 1: it must not be summed)
 *   all-gather of the per-rank body bit totals -> every rank's absolute start bit
 * ghf_comm wraps an ncclComm_t; the RCCL library is bound at first use (dlopen of the copy the process
 * already has, e.g. torch's, else librccl.so.1), so single-GPU users need no RCCL at all.
 * ------------------------------------------------------------------------------------------------ */
typedef struct ghf_comm ghf_comm;
#define GHF_COMM_ID_BYTES 128
int ghf_comm_unique_id(uint8_t id[GHF_COMM_ID_BYTES]);  /* ncclGetUniqueId: one rank calls it, every rank gets the bytes */
int ghf_comm_init_rank(ghf_ctx* ctx, const uint8_t id[GHF_COMM_ID_BYTES], int world, int rank, ghf_comm** out);
int ghf_comm_destroy(ghf_comm* comm);
int ghf_comm_world(const ghf_comm* comm, int* world, int* rank);
int ghf_rccl_version(int* version);                     /* ncclGetVersion of the bound library */
/* the two exchanges, on the context's stream (comm == NULL or world 1: d_totals[0] <- *d_total, nothing else) */
int ghf_comm_allreduce_hist(ghf_ctx* ctx, ghf_comm* comm, uint64_t* d_hist /* [257], in place */);
int ghf_comm_allgather_total(ghf_ctx* ctx, ghf_comm* comm, const uint64_t* d_total, uint64_t* d_totals /* [world] */);
/* This rank's shard of the stream, all of the above in order on the context's stream, no host synchronisation:
 * K1, all-reduce, K2/K3, K4, all-gather, start bit, K5.  rank 0 writes the header and d_out[0] is stream byte 0;
 * rank g > 0 writes from stream byte 16 * (start_bit / 128) on (GHF_EMIT_REBASE); the last rank appends the end mark.
 * cap >= ghf_shard_bound(n): a shard is packed with the GLOBAL code, which may be far from optimal for it.
 * d_code <- the (identical on every rank) tables; *d_start_bit <- this shard's absolute first bit;
 * d_end[0..1] <- {absolute end bit, bytes defined in d_out}; index (optional) <- side-car for ghf_decode of the shard
 * (index->flags is set: GHF_INDEX_NO_END_MARK on every rank but the last). */
int ghf_encode_sharded(ghf_ctx* ctx, ghf_comm* comm, const uint8_t* d_in, size_t n, uint8_t* d_out, size_t cap,
                       ghf_code* d_code, ghf_index* index, uint64_t* d_start_bit, uint64_t* d_end);
size_t ghf_shard_bound(size_t n); /* header + 4 n (32 bits per symbol) + end mark + alignment slack: what fits ANY code */
/* The EXACT number of bytes this rank's K5 will define in d_out, from the all-gathered bit totals (ghf_comm_allgather_total)
 * and the global code -- both known before K5 runs.  A caller that can afford ONE host synchronisation per stream (the first
 * step of a pipeline, or a caller that is not pipelined) sizes its shard outputs with this instead of ghf_shard_bound: at
 * BASELINE config 4 (4 GiB of uniform bytes per rank) that is 4.3 GB per buffer instead of 17.2.  Waits for the context's
 * stream.  *bytes = what ghf_encode_emit / ghf_encode_sharded need as `cap` (whole 16-byte units, the one a shard shares with
 * its right neighbour included); the same number K5 reports in d_end[1] afterwards, rounded up to its last unit. */
int ghf_shard_bytes(ghf_ctx* ctx, const ghf_code* d_code, const uint64_t* d_totals, int world, int rank, size_t* bytes);

/* ------------------------------------------------------------------------------------------------
 * inputs on which the reference is undefined because a code would be longer than 32 bits
 * (include/canonical_huff_encoder.h:43-44; needs > 14.9 M bytes with Fibonacci-like counts).  With GHF_CODE_LIMIT
 * the code lengths are then replaced by the OPTIMAL lengths under a 32-bit limit (package-merge; leaves ordered by
 * (count ascending, byte value ascending), a leaf before a package of equal weight), and the usual canonical
 * assignment (include/canonical_huff_encoder.cc:69-141) follows: the result is an ordinary .crs2 that the
 * reference's decoders read.  Whenever the reference-exact code fits 32 bits the flag changes nothing, so the
 * default output stays bit-exact.
 * ------------------------------------------------------------------------------------------------ */
#define GHF_CODE_LIMIT 1u
/* Opt-in, second half of N4: the EMPTY input.  The reference is undefined there (its merge loop, include/
 * canonical_huff_encoder.cc:309-343, runs n - 1 = 0 times over the lone end mark and leaves every length 0).  With
 * GHF_EMPTY_OK, ghf_build_code_ex gives the end mark the one-bit code "0" (min_len = max_len = 1) and ghf_compress_ex
 * (n == 0) writes the 1048-byte header of that code followed by the byte 0x7F (the end mark, then 1-bits up to the
 * byte, as flush_bits pads): 1049 bytes that ghf_parse_header accepts and ghf_decode turns back into nothing.
 * This is the builder's own definition -- PARITY UNPINNED: no reference output exists to compare with.  The staged
 * calls take n == 0 with any code (that is a rank whose shard is empty in ghf_encode_sharded, which takes it too):
 * ghf_encode_plan gives 0 body bits, and ghf_encode_emit writes what surrounds an empty body -- the header under
 * GHF_EMIT_HEADER, the end mark and its padding at the start bit under GHF_EMIT_LAST (zeros in front of it in its unit
 * under GHF_EMIT_REBASE) -- and always d_end. */
#define GHF_EMPTY_OK 2u
int ghf_build_code_ex(ghf_ctx* ctx, const uint64_t* d_hist, ghf_code* d_code, unsigned flags);
int ghf_compress_ex(ghf_ctx* ctx, const uint8_t* d_in, size_t n, uint8_t* d_out, size_t cap, uint64_t* d_out_bytes,
                    ghf_code* d_code, const ghf_index* index, unsigned code_flags);

/* ------------------------------------------------------------------------------------------------
 * the `.crs` format -- Compressor<NormalHuffEncoder<>> / Decompressor<NormalHuffDecoder<>>
 * (include/normal_huff_encoder.h, include/huff_tree.h, include/huff_tree.cc).  Same histogram (256 byte values,
 * no end mark), the Huffman TREE itself defines the codes ('0' = left = first popped, '1' = right), the file is
 *   [tree in preorder, 2 bytes per node: (0, key) leaf / (255, 255) parent] [left_bits] [last byte] [whole body bytes]
 * The kernels are the ones above (K1, K4, K5, K7, K6); only the code assignment and the framing differ.
 * The reference keeps codes as strings of any length (include/huff_tree.cc:157-170): a tree deeper than 32 -- more than
 * 3.5 M input bytes with counts arranged like Fibonacci numbers -- is packed by a second, slower kernel
 * (GHF_EMIT_LONG_CODES) and decoded by a 64-bit tree walk.  Depths beyond 64 (> 2^44 input bytes) are refused
 * (GHF_E_CODELEN).
 * ------------------------------------------------------------------------------------------------ */

/* The tree as NormalHuffEncoder builds it (EncodeHuffTree, include/huff_tree.h:175-262) and NormalHuffDecoder
 * rebuilds it (DecodeHuffTree::do_build_tree, include/huff_tree.cc:289-303).  Node ids: 0..255 = leaf with that
 * key, 256 + i = the i-th parent; left[i] / right[i] are the children of parent i. */
typedef struct ghf_tree {
  uint16_t left[256];
  uint16_t right[256];
  uint32_t root;        /* node id; >= 256 (a tree that is a single leaf is refused) */
  uint32_t n_leaves;    /* 2 .. 256 */
  uint32_t max_len;     /* depth of the deepest leaf, <= 64 */
  uint32_t tree_bytes;  /* 2 * (2 * n_leaves - 1) */
  uint8_t header[1024]; /* the preorder serialisation (tree_bytes of it), huff_tree.cc:174-187 */
} ghf_tree;

/* EncodeHuffTree::build_tree + gen_encode + serialize_tree (include/huff_tree.cc:138-187) on one wavefront.
 * d_hist: ghf_histogram()'s output (slot [256] is ignored).  d_code receives length[] / codeword[] for K4/K5; when the
 * tree is deeper than 32, codeword[] holds bits 0..31 of every code and symbol[] bits 32..63 (else symbol[] = 0xFFFFFFFF).
 * The counts' domain is the one stated at ghf_build_code, over the 256 counts read here: a sum of 2^GHF_HIST_TOTAL_BITS or
 * more latches GHF_E_INVAL, and neither d_tree nor d_code is written. */
int ghf_crs_build_code(ghf_ctx* ctx, const uint64_t* d_hist, ghf_tree* d_tree, ghf_code* d_code);

/* Compressor<NormalHuffEncoder<>>::compress() (include/compressor.h:62-73, normal_huff_encoder.h:136-186).
 * d_out_bytes <- size of the .crs image.  If the body ends inside a byte, that byte (zero-filled) is ALSO left in
 * d_out right behind the image, which is the layout ghf_crs_decode() wants.  d_tree (optional) receives the tree. */
int ghf_crs_compress(ghf_ctx* ctx, const uint8_t* d_in, size_t n, uint8_t* d_out, size_t cap, uint64_t* d_out_bytes,
                     ghf_tree* d_tree, const ghf_index* index);
size_t ghf_crs_compress_bound(size_t n);

/* DecodeHuffTree::build_tree (include/huff_tree.cc:289-303) on the host, with the checks the reference lacks
 * (truncated / over-long / degenerate trees -> GHF_E_FORMAT, depth > 64 -> GHF_E_CODELEN).  *tree_bytes <- size of
 * the serialised tree; the two prefix bytes {left_bits, last byte} follow it (normal_huff_encoder.h:163-164). */
int ghf_crs_parse_header(const uint8_t* h_stream, size_t n, ghf_tree* tree, size_t* tree_bytes);

/* Decompressor<NormalHuffDecoder<>>::decompress() (include/huff_tree.cc:191-207,255-271).
 * d_stream / stream_bytes: the .crs image from its first byte, with -- when left_bits != 0 -- the stored last byte
 * appended behind the body (so that the code bits are contiguous); stream_bytes counts that byte.
 * index == NULL: the side-car is rebuilt on the GPU (K6) and the stream must end exactly on a code boundary,
 * left_bits bits before its last byte ends.
 * Errors are latched as for ghf_decode: behind GHF_E_FORMAT (a malformed d_tree) nothing is written; GHF_E_CORRUPT from a
 * segment that does not end where the side-car says is found behind that segment's stores, so d_out[0 .. n_symbols) may
 * hold decoded bytes then (never a byte behind them).  GHF_E_CORRUPT from K6 comes before anything is decoded. */
int ghf_crs_decode(ghf_ctx* ctx, const uint8_t* d_stream, size_t stream_bytes, int left_bits, const ghf_tree* d_tree,
                   const ghf_index* index, uint8_t* d_out, size_t cap, uint64_t* d_out_bytes);
int ghf_crs_decoded_size(ghf_ctx* ctx, const uint8_t* d_stream, size_t stream_bytes, int left_bits, const ghf_tree* d_tree,
                         uint64_t* n_out);
/* A .crs body in pieces (the file pipeline of the host layer; the format has no sync points and no end mark either):
 * as ghf_sync_piece, with the tree instead of canonical tables.  d_piece: the piece's own bytes + >= 8 bytes of
 * look-ahead (for the last piece: the stored last byte, then zeros); end_bit = 8 * own bytes, for the last piece minus
 * left_bits of the stored byte that was appended.  landing = where the next piece's first code begins (the last piece
 * must land on 0: the stream ends on a code boundary); n_symbols = codes that start in [first_bit, end_bit).
 * ghf_crs_decode(d_piece, piece_bytes, 0, d_tree, NULL, ...) then decodes the piece with the side-car this call rebuilt. */
int ghf_crs_sync_piece(ghf_ctx* ctx, const uint8_t* d_piece, size_t piece_bytes, uint32_t first_bit, uint64_t end_bit,
                       const ghf_tree* d_tree, uint64_t* landing, uint64_t* n_symbols);

/* ---- an element range of zero-suppressed byte planes: rank tables, range decode ---
 * The sparse form (the next section) stores a plane as a mask and its non-zero bytes.  The values of elements
 * [first, first + count) stand in the values string at offset rank(first), the number of non-zero bytes in front of
 * `first`, and nothing stored says what that is.  THE RANK TABLE of a string of n bytes says it for every multiple of
 * GHF_SPARSE_RANK_ELEMS = 32768 elements -- 4096 mask bytes, exactly one 4096-symbol seek block of the mask's stream.
 * With nb = ceil(n / 32768), little-endian:
 *   64-byte header: "GHFRANK1", u32 version = 1, u32 block_elems = 32768, u64 n, u64 n_vals, u64 n_blocks = nb, zeros;
 *   u64 cum[nb + 1]: cum[j] = the non-zero bytes of x[0 .. 32768 j); cum[0] = 0, cum[nb] = n_vals.
 * 64 + 8 (nb + 1) bytes, 0.024 % of a plane.  It is persistent (the caller stores it beside the images) and NOT TRUSTED:
 * the parse checks what can be checked without the mask; a range call checks the DIFFERENCE of the two entries it reads
 * against the mask's set bits and nothing more.  Two entries wrong by the same amount pass, and the range then returns
 * wrong bytes with GHF_OK: the table guards against damage, not against a forger.
 * Every device pointer is 16-byte aligned unless said otherwise.  The range calls never synchronise. */
#define GHF_SPARSE_RANK_ELEMS 32768u
typedef struct ghf_sparse_rank_info {
  uint64_t n, n_vals, n_blocks;
  uint32_t version, reserved;
} ghf_sparse_rank_info;

/* No reference counterpart (a size the flat buffers of include/compressor.h:62-73 do not need).  Host only:
 * 64 + 8 * (ceil(n / 32768) + 1), the bytes of the rank table of a string of n bytes. */
size_t ghf_sparse_rank_bytes(size_t n);

/* No reference counterpart (an index into the flat input of include/compressor.h:62-73).  Asynchronous on the stream,
 * never synchronises: the mask of a string of n bytes (d_mask, device) -> its rank table image at d_table (device, cap
 * >= ghf_sparse_rank_bytes of n, else GHF_E_CAP); the caller brings it to the host with ghf_copy_d2h.  Three launches in
 * the shape of the sparse split -- popcounts per workgroup slab, the scan, a write pass -- and no kernel waits for
 * another workgroup.  A null pointer, misalignment: GHF_E_INVAL; n == 0: GHF_E_EMPTY.  A set pad bit in the last mask
 * byte latches GHF_E_CORRUPT; behind a latched status nothing is stored. */
int ghf_sparse_rank_pack(ghf_ctx* ctx, const uint8_t* d_mask, size_t n, uint8_t* d_table, size_t cap);

/* No reference counterpart (validates an index into the flat output of include/compressor.h:87-92).  Host only, no GPU,
 * nothing queued: h_table[0 .. bytes) is the whole table.  GHF_E_FORMAT: a wrong magic, version or block size; n_blocks
 * or `bytes` other than n implies; a non-zero reserved byte; cum[0] != 0; a cum that decreases; a step above 32768, or
 * above the elements of the last block; cum[nb] != n_vals.  *info <- n, n_vals, n_blocks, version. */
int ghf_sparse_rank_parse(const uint8_t* h_table, size_t bytes, ghf_sparse_rank_info* info);

/* No reference counterpart (generalises the flat output of include/compressor.h:87-92).  The sparse merge of the next
 * section with the values at d_vals[vals_skip .. vals_skip + n_vals): d_vals stays 16-byte aligned, vals_skip is
 * arbitrary.  Nothing outside d_vals[vals_skip & ~15 .. vals_skip + n_vals), rounded up to the vector that holds the
 * last value, is read.  Every guarantee carries over: only d_out[0 .. n) is written; a launch that finds the status word
 * non-zero stores nothing; set bits that do not number n_vals, or a set pad bit, latch GHF_E_CORRUPT and nothing is
 * stored.  Refusals as there, and vals_skip + n_vals beyond size_t: GHF_E_INVAL. */
int ghf_sparse_merge_at(ghf_ctx* ctx, const uint8_t* d_mask, const uint8_t* d_vals, size_t vals_skip, size_t n_vals, size_t n,
                        uint8_t* d_out);

/* No reference counterpart: Compressor::compress(), include/compressor.h:62-73, once per stored stream, and the rank
 * table of every sparse plane.  The sparse compress of the next section -- images, sizes, codes, side-cars,
 * *h_sparse_planes, h_n_vals and the ONE host wait are byte for byte its own -- plus: d_ranks (device) has elem_bytes
 * slots of rank_slot_bytes (a multiple of 16, >= ghf_sparse_rank_bytes of n_elems, else GHF_E_CAP; a null or
 * misaligned d_ranks: GHF_E_INVAL).  Slot p receives the table of plane p if the plane is stored sparse, queued behind
 * the plane's split while its mask is still in the workspace; slots of dense planes stay unwritten. */
int ghf_compress_planes_sparse_ranked(ghf_ctx* ctx, const uint8_t* d_in, size_t n_elems, uint32_t elem_bytes, unsigned sparse_planes,
                                      uint8_t* d_out, size_t slot_bytes, uint64_t* d_out_bytes /* [2 * elem_bytes] */,
                                      ghf_code* d_codes /* [2 * elem_bytes], optional OUT */,
                                      ghf_index* h_indexes /* [2 * elem_bytes], optional OUT */, unsigned* h_sparse_planes /* OUT */,
                                      size_t* h_n_vals /* [elem_bytes] OUT */, uint8_t* d_ranks, size_t rank_slot_bytes);

/* No reference counterpart: Compressor::compress(), include/compressor.h:62-73, once per stored stream of the byte planes
 * of d_in ^ d_base, and the rank table of every sparse plane.  The call above with the XOR in the histogram and split
 * kernels.  A null or misaligned d_base: GHF_E_INVAL. */
int ghf_compress_planes_sparse_ranked_delta(ghf_ctx* ctx, const uint8_t* d_in, const uint8_t* d_base, size_t n_elems,
                                            uint32_t elem_bytes, unsigned sparse_planes, uint8_t* d_out, size_t slot_bytes,
                                            uint64_t* d_out_bytes /* [2 * elem_bytes] */,
                                            ghf_code* d_codes /* [2 * elem_bytes], optional OUT */,
                                            ghf_index* h_indexes /* [2 * elem_bytes], optional OUT */,
                                            unsigned* h_sparse_planes /* OUT */, size_t* h_n_vals /* [elem_bytes] OUT */,
                                            uint8_t* d_ranks, size_t rank_slot_bytes);

/* No reference counterpart: Decompressor::decompress(), include/compressor.h:87-92, for a part of a typed tensor stored
 * sparse.  d_out[0 .. count * elem_bytes) receives elements [first, first + count).  Asynchronous, never synchronises,
 * from side-cars or from seek tables.  The arrays of 2 * elem_bytes entries are indexed like the slots of the sparse
 * compress: j < elem_bytes is plane j or its mask, elem_bytes + p the values of plane p.  Exactly one source of block
 * starts is given, by the rule of ghf_decode_planes_range: indexes, or (h_infos, h_table_ptrs, h_table_bytes) with the
 * seek-table images in DEVICE memory.  h_rank_infos / h_rank_ptrs (HOST [elem_bytes]): the parsed rank table of every
 * sparse plane and its image in HOST memory; entries of dense planes are not looked at, and both may be NULL when
 * sparse_planes is 0 -- the call is then ghf_decode_planes_range on the same images.
 * THE PLAN with a sparse plane: the common origin is from = first - first % 32768; b0 = from / 32768, b1 = ceil((first
 * + count) / 32768).  A dense plane is decoded from `from` as ghf_decode_planes_range does it.  A sparse plane reads
 * v_lo = cum[b0] and v_hi = cum[b1] on the host, decodes mask bytes [4096 b0, min(4096 b1, mask bytes)) and, if v_hi >
 * v_lo, values [v_lo - v_lo % 4096, v_hi) -- both begin on a seek block -- and ghf_sparse_merge_at (vals_skip = v_lo %
 * 4096, n_vals = v_hi - v_lo, n = min(32768 b1, n_elems) - from) writes the plane into the plane workspace: its count
 * check holds v_hi - v_lo, not the entries themselves, against the mask.  ghf_planes_merge_range comes last and stores nothing behind a
 * latched status.  At most 32767 elements per plane are decoded in front of the range and 32767 behind it.  From seek
 * tables ONE launch expands the covered blocks of all stored streams.
 * Checked before anything is queued, in the order of ghf_decode_planes_range (with n_elems the argument), then:
 * GHF_SPARSE_AUTO or a bit at or above elem_bytes, a null rank pointer of a sparse plane, a rank info whose n is not
 * n_elems, a dense stream whose symbol count is not n_elems, a mask stream whose count is not ghf_sparse_mask_bytes of
 * n_elems, a values stream whose count is not the rank table's n_vals (its pointers, index and table are checked like a
 * plane's; the slot is ignored when n_vals == 0): GHF_E_INVAL; then count == 0: GHF_OK, nothing queued; then the two cum
 * entries read not ordered, above n_vals, or further apart than the sub-string has elements: GHF_E_FORMAT. */
int ghf_decode_planes_sparse_range(ghf_ctx* ctx, const uint8_t* const* h_stream_ptrs /* [2 * elem_bytes] */,
                                   const size_t* h_stream_bytes /* [2 * elem_bytes] */, const ghf_code* d_codes /* [2 * elem_bytes] */,
                                   const ghf_index* indexes /* [2 * elem_bytes] or NULL */,
                                   const ghf_seek_info* h_infos /* [2 * elem_bytes] or NULL */,
                                   const uint8_t* const* h_table_ptrs /* [2 * elem_bytes] or NULL */,
                                   const size_t* h_table_bytes /* [2 * elem_bytes] or NULL */,
                                   const ghf_sparse_rank_info* h_rank_infos /* [elem_bytes] */,
                                   const uint8_t* const* h_rank_ptrs /* [elem_bytes] */, unsigned sparse_planes, size_t n_elems,
                                   uint32_t elem_bytes, uint64_t first, uint64_t count, uint8_t* d_out, size_t cap);

/* No reference counterpart: Decompressor::decompress(), include/compressor.h:87-92, for a part of a typed tensor stored
 * sparse against a base.  The call above with ghf_planes_merge_range_delta last: d_base[0 .. count * elem_bytes) holds
 * the caller's shard of the base, indexed like d_out, and d_base == d_out is allowed; behind a latched status d_out then
 * still holds the base. */
int ghf_decode_planes_sparse_range_delta(ghf_ctx* ctx, const uint8_t* const* h_stream_ptrs /* [2 * elem_bytes] */,
                                         const size_t* h_stream_bytes /* [2 * elem_bytes] */,
                                         const ghf_code* d_codes /* [2 * elem_bytes] */,
                                         const ghf_index* indexes /* [2 * elem_bytes] or NULL */,
                                         const ghf_seek_info* h_infos /* [2 * elem_bytes] or NULL */,
                                         const uint8_t* const* h_table_ptrs /* [2 * elem_bytes] or NULL */,
                                         const size_t* h_table_bytes /* [2 * elem_bytes] or NULL */,
                                         const ghf_sparse_rank_info* h_rank_infos /* [elem_bytes] */,
                                         const uint8_t* const* h_rank_ptrs /* [elem_bytes] */, const uint8_t* d_base,
                                         unsigned sparse_planes, size_t n_elems, uint32_t elem_bytes, uint64_t first, uint64_t count,
                                         uint8_t* d_out, size_t cap);

/* ---- zero-suppressed byte planes: sparse split / merge, compress, decode --------
 * No symbol of a Huffman code costs less than one bit, so a byte plane of nothing but zeros -- the high planes of
 * `new ^ base` in a series of tensors, a frozen layer -- still stores n / 8 bytes.  THE SPARSE FORM of a byte string
 * x[0 .. n) is two byte strings and nothing else (no container, no magic, no header):
 *   mask: ghf_sparse_mask_bytes(n) = (n + 7) / 8 bytes; bit k & 7 of mask[k >> 3] is 1 exactly when x[k] != 0 (LSB first:
 *         numpy's packbits(x != 0, bitorder="little")); the bits behind n in the last mask byte are 0;
 *   vals: the n_vals non-zero bytes of x, in order.
 * Each is compressed as ghf_compress compresses any byte string: EVERY STORED STREAM IS AN ORDINARY STANDALONE .crs2
 * IMAGE.  The mask of such a plane is almost all 0x00 and costs one bit per MASK byte, 1/64 byte per element.
 *
 * Every device pointer is 16-byte aligned (d_n_vals: 8-byte).  Call-level refusals come before anything touches HIP, with
 * nothing queued, in the order of the byte-plane calls: a null context or required pointer, another elem_bytes, a
 * misaligned pointer or slot_bytes, a size beyond size_t, a sparse_planes with a bit at or above elem_bytes,
 * GHF_SPARSE_AUTO together with an explicit bit, GHF_SPARSE_AUTO in a decode (which is told what was chosen), an index
 * that does not carry its stream's symbol count: GHF_E_INVAL; then n == 0: GHF_E_EMPTY; then slot_bytes or cap too small:
 * GHF_E_CAP.  In the decodes d_base == d_out is allowed, as in ghf_decode_planes_delta; any other overlap is undefined. */
#define GHF_SPARSE_AUTO 0x80000000u

/* No reference counterpart (a size the flat buffers of include/compressor.h:62-73 do not need).  Host only:
 * (n + 7) / 8, the bytes of the mask of a string of n bytes. */
size_t ghf_sparse_mask_bytes(size_t n);

/* No reference counterpart (generalises the flat input of include/compressor.h:62-73).  Asynchronous on the stream, never
 * synchronises, does not look at the context's status word.  d_in[0 .. n) -> d_mask[0 .. ghf_sparse_mask_bytes(n)),
 * d_vals[0 .. n_vals), *d_n_vals (device u64) <- n_vals; nothing else is written.  Three launches (count, scan, move): no
 * kernel waits for another workgroup.  n_vals is known on the device behind the scan: n_vals > vals_cap latches GHF_E_CAP,
 * d_vals then stays untouched while d_mask and *d_n_vals -- the capacity that would have sufficed -- are written.  d_vals
 * may be null when vals_cap is 0. */
int ghf_sparse_split(ghf_ctx* ctx, const uint8_t* d_in, size_t n, uint8_t* d_mask, uint8_t* d_vals, size_t vals_cap,
                     uint64_t* d_n_vals);

/* No reference counterpart (generalises the flat output of include/compressor.h:87-92).  The inverse of ghf_sparse_split:
 * only d_out[0 .. n) is written.  Asynchronous, never synchronises.  A launch that finds the context's status word
 * non-zero stores nothing.  Set bits among the first n that do not number n_vals, or a set pad bit, latch GHF_E_CORRUPT
 * and nothing is stored.  The value bytes are not inspected: a zero among them is copied.  n_vals == 0 is allowed and
 * d_vals may then be null. */
int ghf_sparse_merge(ghf_ctx* ctx, const uint8_t* d_mask, const uint8_t* d_vals, size_t n_vals, size_t n, uint8_t* d_out);

/* No reference counterpart: Compressor::compress(), include/compressor.h:62-73, once per stored stream of the byte planes
 * of d_in.  d_out has 2 * elem_bytes slots of slot_bytes >= ghf_planes_slot_bytes(n_elems).  Slot p holds plane p's image
 * if the plane is dense, the image of its MASK if it is sparse; slot elem_bytes + p holds the image of its VALUES, or
 * nothing (d_out_bytes[elem_bytes + p] = 0, the slot unwritten) when the plane is dense or has no non-zero byte.  Every
 * image is byte for byte what ghf_compress writes for that byte string, d_out_bytes[j] (device u64[2 * elem_bytes]) its
 * size and d_codes[j] (device [2 * elem_bytes], optional) its code.
 * sparse_planes: bit p set = plane p is stored sparse; or GHF_SPARSE_AUTO: plane p is sparse when at least n_elems -
 * n_elems / 4 of its bytes are zero.  That is a rule, not a minimum: the second stream has a header of its own, and for
 * a few thousand elements it can outweigh the gain.  *h_sparse_planes (HOST) <- the planes stored sparse, h_n_vals[p]
 * (HOST [elem_bytes]) <- the non-zero bytes of plane p, of every plane: both are what the decode must be told.
 * The call SYNCHRONISES with the host ONCE: it queues ghf_histogram_planes into counters of the context and waits for
 * the elem_bytes x 257 counts, which give h_n_vals and the choice.  Everything behind that is queued without a further
 * wait: ghf_planes_split into the workspace; for a dense plane what ghf_compress_planes_coded(GHF_PLANES_BUILD_CODES)
 * queues; for a sparse plane ghf_sparse_split into a second workspace of the context that grows on demand, then what
 * ghf_compress queues for the mask and for the values.
 * h_indexes (HOST [2 * elem_bytes], optional OUT): the call itself runs ghf_index_alloc for every stream it stores, with
 * that stream's symbol count (n_elems, ghf_sparse_mask_bytes(n_elems) or h_n_vals[p]), and the side-car is filled;
 * entries of empty slots are zeroed.  The caller frees them with ghf_index_free.
 * Device failures latch as for ghf_compress_planes_coded (d_out_bytes UNSPECIFIED behind a latched status); the context's
 * plan and histogram caches are forgotten as there. */
int ghf_compress_planes_sparse(ghf_ctx* ctx, const uint8_t* d_in, size_t n_elems, uint32_t elem_bytes, unsigned sparse_planes,
                               uint8_t* d_out, size_t slot_bytes, uint64_t* d_out_bytes /* [2 * elem_bytes] */,
                               ghf_code* d_codes /* [2 * elem_bytes], optional OUT */,
                               ghf_index* h_indexes /* [2 * elem_bytes], optional OUT */, unsigned* h_sparse_planes /* OUT */,
                               size_t* h_n_vals /* [elem_bytes] OUT */);

/* No reference counterpart: Compressor::compress(), include/compressor.h:62-73, once per stored stream of the byte planes
 * of d_in ^ d_base.  ghf_compress_planes_sparse with ghf_histogram_planes_delta and
 * ghf_planes_split_delta in front; SYNCHRONISES ONCE as it does.  A null or misaligned d_base: GHF_E_INVAL. */
int ghf_compress_planes_sparse_delta(ghf_ctx* ctx, const uint8_t* d_in, const uint8_t* d_base, size_t n_elems, uint32_t elem_bytes,
                                     unsigned sparse_planes, uint8_t* d_out, size_t slot_bytes,
                                     uint64_t* d_out_bytes /* [2 * elem_bytes] */, ghf_code* d_codes /* [2 * elem_bytes], optional OUT */,
                                     ghf_index* h_indexes /* [2 * elem_bytes], optional OUT */, unsigned* h_sparse_planes /* OUT */,
                                     size_t* h_n_vals /* [elem_bytes] OUT */);

/* No reference counterpart: Decompressor::decompress(), include/compressor.h:87-92, once per stored stream.  sparse_planes
 * and h_n_vals (HOST [elem_bytes]; read for the sparse planes) are what the compress call reported.  A dense plane
 * decodes exactly as in ghf_decode_planes.  A sparse plane decodes its mask (ghf_sparse_mask_bytes(n_elems) symbols) and,
 * if h_n_vals[p] > 0, its values into the second workspace; ghf_sparse_merge then writes the plane into the plane
 * workspace.  The merge into d_out comes last and stores nothing behind a latched status.  Codes and pointers of empty
 * slots are ignored.
 * indexes != NULL (HOST [2 * elem_bytes]): the call never synchronises; the index of every stored stream must carry that
 * stream's symbol count, GHF_E_INVAL otherwise, nothing queued.  indexes == NULL SYNCHRONISES per stream as
 * ghf_decode_planes does; a stream that decodes to another size: GHF_E_CORRUPT is returned before any merge. */
int ghf_decode_planes_sparse(ghf_ctx* ctx, const uint8_t* const* h_stream_ptrs /* [2 * elem_bytes] */,
                             const size_t* h_stream_bytes /* [2 * elem_bytes] */, const ghf_code* d_codes /* [2 * elem_bytes] */,
                             const ghf_index* indexes /* [2 * elem_bytes] or NULL */, unsigned sparse_planes,
                             const size_t* h_n_vals /* [elem_bytes] */, size_t n_elems, uint32_t elem_bytes, uint8_t* d_out, size_t cap,
                             uint64_t* d_out_bytes);

/* No reference counterpart: Decompressor::decompress(), include/compressor.h:87-92, once per stored stream.
 * ghf_decode_planes_sparse with ghf_planes_merge_delta last: d_out <- the planes, XOR d_base.  d_base == d_out is allowed;
 * behind a latched status d_out then still holds the base.  indexes == NULL SYNCHRONISES as there. */
int ghf_decode_planes_sparse_delta(ghf_ctx* ctx, const uint8_t* const* h_stream_ptrs /* [2 * elem_bytes] */,
                                   const size_t* h_stream_bytes /* [2 * elem_bytes] */, const ghf_code* d_codes /* [2 * elem_bytes] */,
                                   const ghf_index* indexes /* [2 * elem_bytes] or NULL */, const uint8_t* d_base, unsigned sparse_planes,
                                   const size_t* h_n_vals /* [elem_bytes] */, size_t n_elems, uint32_t elem_bytes, uint8_t* d_out,
                                   size_t cap, uint64_t* d_out_bytes);

#ifdef __cplusplus
}
#endif

/* ---- one stored object per typed tensor: the container GHFTENS1 ----------------------------
 * Everything above stores a typed tensor as slots, device sizes, codes, side-cars, rank tables, two masks and value counts
 * that the caller keeps.  The calls of this section keep all of it in ONE contiguous, self-describing, relocatable image:
 * bound, pack, compress, workspace release, parse, open, close, describe, decode, range decode and gather of a tensor container.  No
 * reference counterpart.  The declarations stand in include/ghf_tensor.h, which this header includes here, as their
 * binding stands in a Python module of its own (golden-huffman_amd/ghf_tensor.py) beside the recorded one. */
#include "ghf_tensor.h"

#endif /* GHF_H_ */
