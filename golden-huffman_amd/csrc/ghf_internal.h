// golden-huffman_amd/csrc/ghf_internal.h -- shared between the HIP kernels and the C-ABI host layer.
#ifndef GHF_INTERNAL_H_
#define GHF_INTERNAL_H_
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "ghf.h"

namespace ghf {

// ---- geometry ---------------------------------------------------------------------------------
constexpr int kWave = 64;               // CDNA wavefront
constexpr int kSymPerLane = 16;         // one 16-byte vector load = one lane's contiguous symbols
constexpr int kSymPerIter = kWave * kSymPerLane;  // 1 KiB of input per wave iteration
constexpr int kSegSymbols = 64;         // side-car granularity (4 lanes of K5, one lane of K7)
constexpr int kBlockSymbols = 4096;     // side-car block = 64 segments = one K7 group = 4 K5 tiles; absolute bit per block
// A chunk = the input one K5 wave packs (and the unit K1 prices for K4).  Chunks are sized so that ALL of them are resident
// at once: K5 keeps 3 workgroups x 8 waves on each of the 256 CUs, and a grid of 1.33 rounds (8192 power-of-two chunks, as in
// round 1) spends its last third with a third of the waves -- too few loads in flight to keep HBM busy.  Multiples of
// 4 KiB (K1's vector rows: 256 threads x 16 bytes; K5's trips of four 1 KiB tiles), at least 16 KiB, at most 1 MiB.  (Round 3 tried 2 workgroups x 16 waves, 8 waves per SIMD:
// 3 % faster alone, 12 % slower between the other kernels of the pipelined bench -- a 1024-thread workgroup needs half a
// CU to drain before it can start.)
constexpr uint32_t kChunkQuantum = 4096;
constexpr uint32_t kMinChunk = 16384;
constexpr uint32_t kMaxChunk = 1u << 20;
constexpr uint32_t kEmitSlots = 256 * 3 * 8;

// K1 histogram
constexpr int kHistThreads = 256;
constexpr int kHistRep = 32;  // bins[256][32]: replica = lane % 32 -> every lane of a 32-lane LDS group owns a bank

// K5 emit
constexpr int kEmitThreads = 512;                 // 8 waves share one 32 KiB replicated code table
constexpr int kEmitWaves = kEmitThreads / kWave;
constexpr int kStageWords = 544;                  // per-wave staging: 128 carry bits + 16384 bits + slack
constexpr int kStageCapBits = (kStageWords - 8) * 32;

// K7 decode / K6 side-car reconstruction
constexpr int kDecPairBitsMax = 10;
constexpr int kDecLutBitsMax = 12;
// K7 / K6 keep the direct table in LDS as 32-bit entries, replicated (ghf_dec_core.h): 64 KiB of slots + a small region
constexpr int kDec7LutLog2 = 14;
constexpr int kDec7LutSlots = 1 << kDec7LutLog2;
constexpr int kDec7SmallSlots = 1024;  // pair mode (max_len <= 5): the one-symbol table for ragged tails and the end mark, 32 copies

// byte planes (ghf_planes.hip): one wave = one workgroup moves a tile of 64 * max(E, 4) 16-byte vectors of the interleaved
// side at a time -- 2048 elements of 2 bytes, 1024 of 4 or 8 -- through an LDS tile of its own
constexpr uint32_t kPlanesGroups = 256 * 16;      // one resident round: 16 one-wave workgroups on each of the 256 CUs
constexpr uint32_t kPlanesLdsBytes = 9 * 1024;    // per workgroup: 64 rows of (8 + 1) vectors at E = 8; 6 KiB (E = 2), 5 KiB (E = 4)
__host__ __device__ constexpr inline uint32_t planes_tile_elems(uint32_t elem_bytes) {
  return (uint32_t)kWave * (elem_bytes < 4 ? 4 : elem_bytes) * 16 / elem_bytes;
}
// the launchers' ladder over elem_bytes = 2, 4 or 8 (the callers have checked it): f(std::integral_constant<int, E>())
template <class F>
inline void with_elem_bytes(uint32_t elem_bytes, F&& f) {
  if (elem_bytes == 2) f(std::integral_constant<int, 2>());
  else if (elem_bytes == 4) f(std::integral_constant<int, 4>());
  else f(std::integral_constant<int, 8>());
}
// the one-pass plane histograms (ghf_planes_hist.hip): K1's 32 KiB of u32 counters, bins[256][32], whose
// 32 columns are E planes x 32 / E replicas
constexpr int kPlanesHistThreads = 256;
constexpr int kPlanesHistCols = 32;
constexpr uint32_t kPlanesHistGroups = 256 * 4;    // one resident round: 4 workgroups on each of the 256 CUs, as K1
constexpr uint32_t kPlanesHistTileVecs = kPlanesHistThreads * 4;  // a tile: four 16-byte vectors per thread, 16 KiB
constexpr uint32_t kPlanesHistFlushTiles = 3;      // u32 counters -> u64 sums every 48 KiB of a workgroup's input (K1: every chunk)
static_assert((uint64_t)(kPlanesHistFlushTiles + 1) * kPlanesHistTileVecs * 16 < (1ull << 32), "a u32 counter never wraps between two flushes");
constexpr size_t kPlanesHistAccWords = 32 * GHF_PLANES_MAX * 256;  // 32 replicas of the E x 256 totals, all zero between launches
// zero-suppressed byte strings (ghf_sparse.hip): one wave = one workgroup takes kSparseTile bytes of the
// string at a time, 64 lanes x 4 vectors of 16 bytes; one resident round of workgroups with a contiguous slab of tiles each
constexpr uint32_t kSparseTile = 4096;
constexpr uint32_t kSparseGroups = 256 * 16;       // as kPlanesGroups; also the most counts the one-workgroup scan takes, in ONE step
constexpr uint32_t kSparseLdsBytes = 258 * 16;     // the compacted side of a tile at any byte phase: (15 + 4096 + 15) / 16 + 1 vectors
constexpr size_t kSparseOffWords = kSparseGroups + 2;  // offs[groups] = the total; the last word: n_vals of a split inside a plane call
// the rank table of a sparse string: a 64-byte header, then cum[0 .. blocks] as u64, little-endian;
// cum[j] = the non-zero bytes in front of element kSparseRankElems * j.  A rank block is 4096 mask bytes: one seek block of
// the mask's stream
constexpr uint32_t kSparseRankElems = 32768;
constexpr size_t kSparseRankHeaderBytes = 64;
constexpr uint64_t kSparseRankMagic = 0x314B4E4152464847ull;  // "GHFRANK1"
constexpr uint32_t kSparseRankVersion = 1;
static_assert(kSparseRankElems == 8 * kBlockSymbols, "a rank block of the mask is one seek block");

// the .crs2 header: the count word, symbol[257], min_len, max_len, then a (start_pos, first_code) row per length 1..max_len
constexpr uint64_t kHeaderFixedBytes = 4 * (GHF_NSYM + 3);  // 1040
template <class T>  // in the type of its argument: kernels that count in 32 bits keep doing so
__host__ __device__ constexpr inline T header_bytes_for(T max_len) { return (T)kHeaderFixedBytes + 8 * max_len; }
// the side-car of n symbols: blocks (one absolute bit each) and segments (one relative end bit each)
__host__ __device__ constexpr inline uint64_t blocks_for(uint64_t n) { return (n + kBlockSymbols - 1) / kBlockSymbols; }
__host__ __device__ constexpr inline uint64_t segs_for(uint64_t n) { return (n + kSegSymbols - 1) / kSegSymbols; }
inline void index_shape(uint64_t n, ghf_index* ix) {  // everything of a ghf_index but its flags and its arrays
  ix->n_symbols = n;
  ix->chunk_symbols = kBlockSymbols;
  ix->seg_symbols = kSegSymbols;
  ix->n_chunks = blocks_for(n);
  ix->n_segs = segs_for(n);
}

inline uint32_t chunk_symbols_for(uint64_t n) {
  const uint64_t per_slot = (n + kEmitSlots - 1) / kEmitSlots;
  uint64_t c = (per_slot + kChunkQuantum - 1) / kChunkQuantum * kChunkQuantum;
  if (c < kMinChunk) c = kMinChunk;
  if (c > kMaxChunk) c = kMaxChunk;
  return (uint32_t)c;
}
inline uint64_t chunk_count_for(uint64_t n) {
  const uint64_t c = chunk_symbols_for(n);
  return (n + c - 1) / c;
}

// decode-side tables derived from ghf_code (built on the device by k_build_decode_tables)
struct DecTables {
  uint32_t fc_left[36];    // first_code[len] << (32 - len), len = 1..max_len; 0xFFFFFFFF for len < min_len
  uint32_t start_pos[36];
  uint16_t symbol[GHF_NSYM + 3];
  int32_t min_len, max_len, lut_bits;
  int32_t pair_bits;       // 2 * max_len when that is <= kDecPairBitsMax (every pair of codes fits lut2's index), else 0
  // kind 1 (.crs): the codes are whatever the tree says; codes beyond the direct table are decoded by
  // walking tl/tr (children of parent i; ids < 256 = leaf key, else 256 + parent index) from `root`
  int32_t kind;
  uint32_t root;
  uint16_t tl[256], tr[256];
  // work counters of k_decode, zeroed by k_build_decode_tables.  One word saturates at ~88 tickets/us (measured:
  // a single counter made the 256 MiB decode 4.8x slower), so the workgroups are split into 16 classes
  // (blockIdx % 16), each with its own counter on its own 128-byte line; class c owns the groups == c (mod 16).
  uint32_t ticket[16 * 32];
  // workgroups of the running k_decode that have finished; the last one zeroes the counters again (and this word), so
  // that tables stay usable for any number of launches
  uint32_t done;
  // The direct table(s) exactly as K7 / K6 keep them in LDS (ghf_dec_core.h: 32-bit entries, replicated): written once by the
  // table kernels, pulled in by every workgroup with 16-byte loads (round 3 replicated a compact table in every workgroup's
  // prologue: ~3 us per launch of K7 and of every K6 kernel).  One-symbol table: index = the next lut_bits stream bits,
  //   entry = symbol | length << 8 | bit 16: end mark | bit 17: no code of <= lut_bits bits starts with these bits
  // in min(32, 2^(14 - lut_bits)) copies, slot = index * copies + copy.  Small alphabets (pair_bits != 0): the first 2^14 slots
  // hold the pair table -- index = the next pair_bits bits, entry = sym0 | sym1 << 8 | (len0 + len1) << 16 | bit 30: not two data
  // symbols -- and the one-symbol table follows in 32 copies.
  alignas(16) uint32_t image[kDec7LutSlots + kDec7SmallSlots];
};

struct EmitParams {
  const uint8_t* in;
  uint64_t n;
  const ghf_code* code;
  const uint64_t* chunk_off;  // [nchunks + 1] bits relative to this buffer's first code (exclusive scan)
  const uint64_t* d_start_bit;
  uint8_t* out;
  uint64_t cap;
  uint32_t chunk;       // symbols per chunk (a multiple of 4 KiB, >= 16 KiB)
  uint32_t nchunks;
  uint64_t* chunk_bit;  // side-car (may be null): [n / 4096] absolute start bit of every block
  uint32_t* seg_bit;    // side-car (may be null): [n / 64] end bit of every segment, relative to its block
  int flags;
  int* status;
  uint64_t* d_end;  // may be null
};

struct DecParams {
  const uint8_t* stream;
  uint64_t stream_bytes;
  DecTables* dt;
  const uint64_t* chunk_bit;
  const uint32_t* seg_bit;
  uint64_t n_symbols;
  uint64_t n_segs;
  uint32_t no_end_mark;  // the last symbol is not followed by the end mark (a shard that is not the stream's last)
  uint8_t* out;
  uint64_t* out_bytes;  // optional device u64 <- n_symbols
  int* status;
};

// ---- the seek table: the persistent form of the side-car (DESIGN.md "Seekable .crs2") ---------------------------------
// 64-byte header, then one 24-byte record per block: u64 start_bit (= chunk_bit), u16 run_bits[8] (bit lengths of the
// block's eight runs of 512 symbols).  All little-endian.
constexpr int kRunSymbols = 512;
constexpr int kRunsPerBlock = kBlockSymbols / kRunSymbols;  // 8
constexpr int kRunSegs = kRunSymbols / kSegSymbols;         // 8
constexpr size_t kSeekHeaderBytes = 64;
constexpr size_t kSeekRecordBytes = 24;
constexpr uint64_t kSeekMagic = 0x314B454553464847ull;  // "GHFSEEK1"
constexpr uint32_t kSeekVersion = 1;

struct SeekPackParams {
  const uint64_t* chunk_bit;
  const uint32_t* seg_bit;
  uint64_t n_symbols, n_blocks, n_segs;
  uint32_t flags;
  uint8_t* table;  // 16-byte aligned, kSeekHeaderBytes + n_blocks * kSeekRecordBytes
  int* status;
};
// blocks [g0, g1) of the table -> chunk_bit[0 .. g1 - g0), seg_bit[0 .. 64 * (g1 - g0)) (only the segments that exist)
struct SeekExpandParams {
  const uint8_t* records;  // the table behind its header: 8-byte aligned, n_blocks records
  const uint8_t* stream;
  uint64_t stream_bytes;
  const DecTables* dt;
  uint64_t n_symbols, n_blocks;  // of the whole stream
  uint64_t g0, g1;
  uint64_t* chunk_bit;
  uint32_t* seg_bit;
  int* status;
};
// the same blocks of up to GHF_PLANES_MAX streams of one n_symbols in one launch: plane[p] as above, with equal g0 and g1
struct SeekExpandPlanesParams {
  SeekExpandParams plane[GHF_PLANES_MAX];
};
// up to kSeekStreamsMax streams in one launch, every one with its own n_symbols, tables and blocks [g0, g1) (the mask and
// values streams of ghf_decode_planes_sparse_range).  16 x 88 bytes: well inside the 4 KiB of kernel arguments
constexpr uint32_t kSeekStreamsMax = 2 * GHF_PLANES_MAX;
struct SeekExpandStreamsParams {
  SeekExpandParams stream[kSeekStreamsMax];
};
static_assert(sizeof(SeekExpandStreamsParams) <= 4096 - 64, "the parameter block stays under the kernel-argument limit");
// the part [lo, hi) of ONE block (hi <= the block's end) -> out[0 .. hi - lo)
struct DecHeadParams {
  const uint8_t* stream;
  uint64_t stream_bytes;
  const DecTables* dt;
  const uint64_t* chunk_bit;  // the block's
  const uint32_t* seg_bit;    // the block's first segment
  uint64_t blk_sym0;          // stream position of the block's first symbol
  uint64_t n_symbols;         // of the whole stream
  uint64_t lo, hi;
  uint8_t* out;
  int* status;
};

// ---- batches of small independent streams (ghf_batch.hip): one workgroup per item; every array is device memory -----
struct BatchCompressParams {
  const uint8_t* const* in_ptrs;
  const uint64_t* in_bytes;
  uint64_t max_item_bytes;
  uint8_t* const* out_ptrs;
  const uint64_t* out_caps;
  uint64_t* out_bytes;
  ghf_code* codes;        // [count], never null (the host driver lends its own when the caller keeps none)
  uint64_t* chunk_bit;    // side-car slices (may both be null): item i at i * blocks_per_item / i * segs_per_item
  uint32_t* seg_bit;
  uint64_t blocks_per_item, segs_per_item;
  int* item_status;
};
struct BatchDecodeParams {
  const uint8_t* const* stream_ptrs;
  const uint64_t* stream_bytes;
  const ghf_code* codes;
  const uint64_t* chunk_bit;
  const uint32_t* seg_bit;
  uint64_t blocks_per_item, segs_per_item;
  uint64_t max_item_bytes;
  const uint64_t* n_symbols;
  uint8_t* const* out_ptrs;
  const uint64_t* out_caps;
  uint64_t* out_bytes;
  int* item_status;
};
// standalone images, nothing else (ghf_decode_images_batch): header, code boundaries and offsets are found by the workgroup
struct BatchImagesParams {
  const uint8_t* const* stream_ptrs;
  const uint64_t* stream_bytes;
  uint64_t max_stream_bytes;  // ghf_compress_bound(GHF_BATCH_MAX_ITEM): the workgroup's bit offsets fit 32 bits
  uint8_t* const* out_ptrs;   // null: sizes only (out_caps is ignored)
  const uint64_t* out_caps;
  uint64_t* out_bytes;
  ghf_code* codes;            // [count], may be null
  int* item_status;
  uint64_t* stats;            // may be null: [0] += rounds, [1] += passes of every item that reached its body
};

// ---- batches under one shared code (ghf_batch_shared.hip): an item's output is its body alone; every array is device memory
struct BatchHistParams {
  const uint8_t* const* in_ptrs;
  const uint64_t* in_bytes;
  uint64_t max_item_bytes;
  uint32_t count;
  uint64_t* hist;  // [GHF_NSYM]; slots 0 .. 255 are zero when the kernel starts
};
struct BatchSharedCompressParams {
  const uint8_t* const* in_ptrs;
  const uint64_t* in_bytes;
  uint64_t max_item_bytes;
  const ghf_code* code;   // one for the batch, never null
  uint8_t* const* out_ptrs;
  const uint64_t* out_caps;
  uint64_t* out_bytes;
  uint64_t* chunk_bit;    // side-car slices (may both be null), bits counted from byte 0 of the item's body
  uint32_t* seg_bit;
  uint64_t blocks_per_item, segs_per_item;
  int* item_status;
};
struct BatchSharedDecodeParams {
  const uint8_t* const* stream_ptrs;  // the bodies
  const uint64_t* stream_bytes;
  const ghf_code* code;
  const uint64_t* chunk_bit;
  const uint32_t* seg_bit;
  uint64_t blocks_per_item, segs_per_item;
  uint64_t max_item_bytes;
  const uint64_t* n_symbols;
  uint8_t* const* out_ptrs;
  const uint64_t* out_caps;
  uint64_t* out_bytes;
  int* item_status;
};
// bodies under one code, nothing else (ghf_decode_bodies_batch_shared): code boundaries and sizes are found by the workgroup
struct BatchSharedBodiesParams {
  const uint8_t* const* stream_ptrs;  // the bodies
  const uint64_t* stream_bytes;
  uint64_t max_stream_bytes;  // ghf_compress_batch_shared_bound(GHF_BATCH_MAX_ITEM): the workgroup's bit offsets fit 32 bits
  const ghf_code* code;       // one for the batch, never null
  uint8_t* const* out_ptrs;   // null: sizes only (out_caps is ignored)
  const uint64_t* out_caps;
  uint64_t* out_bytes;
  int* item_status;
  uint64_t* stats;            // may be null: [0] += rounds, [1] += passes of every item that reached its body
};

// ---- shared-code batches of byte planes (ghf_batch_planes.hip): items of elements of elem_bytes = E bytes, one code per
// byte plane; slot j = i * E + p is plane p of item i.  Every array is device memory
struct BatchPlanesHistParams {
  const uint8_t* const* in_ptrs;
  const uint64_t* in_bytes;
  uint64_t max_item_bytes;
  uint32_t count;
  uint64_t* hists;  // [E][GHF_NSYM]; all zero when the kernel starts
};
struct BatchPlanesCompressParams {
  const uint8_t* const* in_ptrs;  // [count]
  const uint64_t* in_bytes;
  uint64_t max_item_bytes;        // a multiple of E
  const ghf_code* codes;          // [E], never null
  uint8_t* const* out_ptrs;       // [count * E], as are the four below
  const uint64_t* out_caps;
  uint64_t* out_bytes;
  uint64_t* chunk_bit;            // side-car slices per slot (may both be null)
  uint32_t* seg_bit;
  uint64_t blocks_per_item, segs_per_item;
  int* item_status;
};
struct BatchPlanesDecodeParams {
  const uint8_t* const* stream_ptrs;  // [count * E] the bodies
  const uint64_t* stream_bytes;
  const ghf_code* codes;              // [E]
  const uint64_t* chunk_bit;          // slices per slot
  const uint32_t* seg_bit;
  uint64_t blocks_per_item, segs_per_item;
  uint64_t max_plane_symbols;         // what a slice of the index covers
  const uint64_t* n_elems;            // [count], as are the four below
  uint8_t* const* out_ptrs;
  const uint64_t* out_caps;           // bytes
  uint64_t* out_bytes;
  int* item_status;
};
struct BatchPlanesBodiesParams {
  const uint8_t* const* stream_ptrs;  // [count * E] the bodies
  const uint64_t* stream_bytes;
  uint64_t max_stream_bytes;          // as BatchSharedBodiesParams
  const ghf_code* codes;              // [E]
  uint8_t* const* out_ptrs;           // [count]; null: sizes only (out_caps is ignored)
  const uint64_t* out_caps;           // bytes
  uint64_t* out_bytes;
  int* item_status;
  uint64_t* stats;                    // may be null: [0] += rounds, [1] += passes of every plane that reached its body
};

// ---- stored shared-code bodies (ghf_batch_seek.hip): the run record, the persistent form of one
// slice of a ghf_batch_index.  u32 magic, u32 n_symbols, u16 run_bits[ceil(n_symbols / 128)], zeros up to a multiple of 8;
// all little-endian.  A run never straddles a side-car block: 32 runs of two segments each make one.
constexpr uint32_t kBatchSeekMagic = 0x31524247u;  // "GBR1"
constexpr uint32_t kBatchRunSymbols = 128;
constexpr uint32_t kBatchRunSegs = kBatchRunSymbols / kSegSymbols;         // 2
constexpr uint32_t kBatchRunsPerBlock = kBlockSymbols / kBatchRunSymbols;  // 32
constexpr uint32_t kBatchSeekHeadBytes = 8;
__host__ __device__ constexpr inline uint64_t batch_runs_for(uint64_t n) { return (n + kBatchRunSymbols - 1) / kBatchRunSymbols; }
__host__ __device__ constexpr inline uint64_t batch_seek_bytes_for(uint64_t n) {
  return (kBatchSeekHeadBytes + 2 * batch_runs_for(n) + 7) & ~7ull;
}
struct BatchSeekPackParams {
  const uint64_t* chunk_bit;  // the side-car slices, slot j at j * blocks_per_item / j * segs_per_item
  const uint32_t* seg_bit;
  uint64_t blocks_per_item, segs_per_item;
  uint64_t max_slice_symbols;  // what a slice covers
  const uint64_t* in_bytes;    // [count]: slot j holds in_bytes[j / elem_bytes] / elem_bytes symbols
  uint32_t elem_bytes;         // 1, 2, 4 or 8
  uint8_t* const* rec_ptrs;    // [count * elem_bytes], as are the three below
  const uint64_t* rec_caps;
  uint64_t* rec_bytes;
  int* slot_status;
};
// bodies and their records under one code (elem_bytes = 1: item = slot) or one code per byte plane
struct BatchSeekDecodeParams {
  const uint8_t* const* stream_ptrs;  // [count * elem_bytes] the bodies
  const uint64_t* stream_bytes;
  const uint8_t* const* rec_ptrs;     // [count * elem_bytes] the records
  const uint64_t* rec_bytes;
  uint64_t max_stream_bytes;          // as BatchSharedBodiesParams
  const ghf_code* codes;              // [elem_bytes]
  uint8_t* const* out_ptrs;           // [count]; null: sizes only (out_caps is ignored)
  const uint64_t* out_caps;           // bytes
  uint64_t* out_bytes;
  int* item_status;
};

// K6: side-car reconstruction for foreign streams
enum SyncKind : uint32_t {  // what SyncParams::no_eof carries
  kSyncCrs2 = 0,   // a whole .crs2: ends with the end mark
  kSyncCrs = 1,    // a whole .crs: no end mark, the last code must end exactly at end_bit
  kSyncPiece = 2,  // a piece of a stream (multi-GPU / file pipeline): see SyncParams::no_eof
};
struct SyncParams {
  const uint8_t* stream;
  uint64_t stream_bytes;
  uint64_t body_bit0;  // first body bit = 8 * header bytes
  uint64_t end_bit;    // one past the last bit that may belong to a code (8 * stream_bytes for .crs2)
  uint32_t no_eof;     // 0: .crs2, ends with the end mark.  1: .crs, no end mark, the last code must end exactly at end_bit.
                       // 2: a piece of a .crs2 (multi-GPU decode): an end mark ends it if there is one, otherwise the last
                       //    code may run past end_bit and start[nsub] receives by how much
  const DecTables* dt;
  uint64_t nsub;       // 512-bit subsequences covering the body
  uint16_t* start;     // [nsub + 1] current guess: bit offset of the first code boundary inside each subsequence
  uint16_t* used;      // [nsub]     the guess the stored result was computed from (0xFFFF = none yet)
  uint32_t* cnt;       // [nsub]     codes starting in the subsequence (up to an end mark)
  uint8_t* eof;        // [nsub]     the end mark was decoded in this subsequence
  uint32_t first;      // k_sync_pass only.  bit 0: every subsequence has work (`used`, `eof` hold nothing yet: the launch that
                       // writes them all needs no memset in front of it); bit 1: every guess is 0 except subsequence 0's
                       // (`start` holds nothing yet either; this launch writes start[1 .. nsub])
  uint32_t first_start;  // subsequence 0's guess (bit 1 of `first`)
  uint32_t* changed;   // [0] some guess moved during the pass; [1] how many did, roughly (every 256th group counts)
  unsigned long long* moved_first_inv;  // ~(smallest subsequence whose landing moved during the pass); 0: none (sits behind `changed`)
  uint64_t* eof_sub;   // first subsequence holding the end mark
  uint64_t* tile_sum;  // [nsub / 256 + 2] symbols per tile, then (in place) their exclusive scan
};

// ---- kernel launchers; all asynchronous on `s` ---------------------------------------------------------------------------
// ghf_kernels.hip
// K1 scratch, all zero between launches: 32 replicas of the 256 totals, the arrival counter (word 8192), 16 ticket
// counters (word 8208 + 16 k, one 128-byte line each)
constexpr size_t kHistAccWords = 32 * 256 + 16 + 16 * 16;
void launch_histogram(const uint8_t* d_in, uint64_t n, uint32_t chunk, uint32_t nchunks, uint32_t* d_chunk_hist,
                      uint64_t* d_hist, uint64_t* d_acc, bool add, hipStream_t s);
void launch_build_code(const uint64_t* d_hist, ghf_code* d_code, int* d_status, uint32_t flags, hipStream_t s);
void launch_write_header(const ghf_code* d_code, uint8_t* d_out, uint64_t cap, int* d_status, hipStream_t s);
void launch_plan(const uint8_t* d_in, uint64_t n, uint32_t chunk, uint32_t nchunks, const uint32_t* d_chunk_hist,
                 const ghf_code* d_code, uint64_t* d_chunk_off, uint64_t* d_total_bits, hipStream_t s);
// in-place exclusive scan of d_v[0..count), d_v[count] = total, *d_total = total (one workgroup)
void launch_scan(uint64_t* d_v, uint32_t count, uint64_t* d_total, hipStream_t s);
void launch_crs_build_code(const uint64_t* d_hist, ghf_tree* d_tree, ghf_code* d_code, uint64_t* d_start_bit, int* d_status,
                           hipStream_t s);
void launch_crs_finish(const ghf_tree* d_tree, const uint64_t* d_total_bits, uint8_t* d_out, uint64_t* d_out_bytes, int* d_status,
                       hipStream_t s);
void launch_stream_copy(const uint8_t* d_src, uint8_t* d_dst, uint64_t n, bool nt, hipStream_t s);
void launch_store_u64(uint64_t* d_dst, const uint64_t* d_src_opt, uint64_t add, hipStream_t s);
void launch_load_u16(uint64_t* d_dst, const uint16_t* d_src, hipStream_t s);
void launch_shard_start(const ghf_code* d_code, const uint64_t* d_totals, int rank, uint64_t* d_start_bit, hipStream_t s);
// ghf_emit.hip
void launch_emit(const EmitParams& p, hipStream_t s);
// ghf_decode.hip: the decode tables and K7
void launch_build_decode_tables(const ghf_code* d_code, DecTables* d_dt, int* d_status, hipStream_t s);
// d_dts[j] from d_codes[j] for every j < count with bit j of `slots` set, in one launch
void launch_build_decode_tables_slots(const ghf_code* d_codes, DecTables* d_dts, uint32_t count, uint32_t slots, int* d_status, hipStream_t s);
void launch_crs_decode_tables(const ghf_tree* d_tree, DecTables* d_dt, int* d_status, hipStream_t s);
constexpr uint64_t kDecMaxGroups = 0xFFFF0000ull;  // groups of 4096 symbols one k_decode launch takes (2^44 symbols)
void launch_decode(const DecParams& p, hipStream_t s);
// ghf_sync.hip: K6
void launch_sync_pass(const SyncParams& p, hipStream_t s);
void launch_sync_counts(const SyncParams& p, uint64_t* d_total, hipStream_t s);
// deterministic seeding of p.start[] (function-composition scan); ws = sync_scan_workspace(p.nsub) bytes, 256-byte aligned
size_t sync_scan_workspace(uint64_t nsub);
void launch_sync_scan(const SyncParams& p, uint8_t* ws, uint32_t stride /* 16: max_len <= 16 is known; 64: it may exceed 32 (.crs); else 32 */,
                      uint32_t entry /* bit at which the first code begins, < stride */, hipStream_t s);
void launch_sync_index(const SyncParams& p, uint64_t* d_seg_abs, uint64_t n_symbols, uint64_t* d_chunk_bit, uint32_t* d_seg_bit,
                       hipStream_t s);
// ghf_seek.hip: the seek table and the range head
void launch_seek_pack(const SeekPackParams& p, hipStream_t s);
void launch_seek_expand(const SeekExpandParams& p, hipStream_t s);
void launch_seek_expand_planes(const SeekExpandPlanesParams& a, uint32_t planes, hipStream_t s);
// streams whose [g0, g1) is empty take no part; nothing is queued when all are
void launch_seek_expand_streams(const SeekExpandStreamsParams& a, uint32_t streams, hipStream_t s);
void launch_decode_head(const DecHeadParams& p, hipStream_t s);
// ghf_batch.hip
void launch_compress_batch(const BatchCompressParams& p, uint32_t count, hipStream_t s);  // one launch, grid = count
void launch_decode_batch(const BatchDecodeParams& p, uint32_t count, hipStream_t s);
void launch_decode_images_batch(const BatchImagesParams& p, uint32_t count, hipStream_t s);  // one launch; p.out_ptrs null: sizes only
// ghf_batch_shared.hip
void launch_histogram_batch(const BatchHistParams& p, uint32_t flags, hipStream_t s);  // zeroes p.hist, counts, finishes
void launch_compress_batch_shared(const BatchSharedCompressParams& p, uint32_t count, hipStream_t s);  // one launch, grid = count
void launch_decode_batch_shared(const BatchSharedDecodeParams& p, uint32_t count, hipStream_t s);
void launch_decode_bodies_batch_shared(const BatchSharedBodiesParams& p, uint32_t count, hipStream_t s);  // one launch; p.out_ptrs null: sizes only
// d_hists[k][256] <- 1 and, under GHF_HIST_COVER_ALL, every count of 0 <- 1, for k < n_hists (behind the counting kernel)
void launch_histogram_batch_finish(uint64_t* d_hists, uint32_t n_hists, uint32_t flags, hipStream_t s);
// ghf_batch_planes.hip: elem_bytes is 2, 4 or 8
void launch_histogram_batch_planes(const BatchPlanesHistParams& p, uint32_t elem_bytes, uint32_t flags, hipStream_t s);  // zeroes, counts, finishes
void launch_build_codes(const uint64_t* d_hists, uint32_t n_codes, ghf_code* d_codes, int* d_status, uint32_t flags, hipStream_t s);
// d_raw_planes <- the mask the rule picks (bit p = plane p, below elem_bytes)
void launch_batch_planes_raw_auto(const uint64_t* d_hists, const ghf_code* d_codes, uint32_t elem_bytes, uint32_t* d_raw_planes,
                                  hipStream_t s);
// forms: the _forms kernel, with the planes of `raw_planes` stored raw; else the _shared kernel, which takes no mask
void launch_compress_batch_planes(const BatchPlanesCompressParams& p, uint32_t count, uint32_t elem_bytes, bool forms, uint32_t raw_planes,
                                  hipStream_t s);  // grid = count * E
void launch_decode_batch_planes(const BatchPlanesDecodeParams& p, uint32_t count, uint32_t elem_bytes, bool forms, uint32_t raw_planes,
                                hipStream_t s);  // grid = count
void launch_decode_bodies_batch_planes(const BatchPlanesBodiesParams& p, uint32_t count, uint32_t elem_bytes, bool forms,
                                       uint32_t raw_planes, hipStream_t s);
// ghf_batch_seek.hip: elem_bytes is 1 (flat items; no forms), 2, 4 or 8
void launch_batch_seek_pack(const BatchSeekPackParams& p, uint32_t slots, hipStream_t s);  // one launch, grid = slots
// forms: as above; a raw plane has no record
void launch_decode_bodies_batch_seek(const BatchSeekDecodeParams& p, uint32_t count, uint32_t elem_bytes, bool forms, uint32_t raw_planes,
                                     hipStream_t s);  // grid = count
// ghf_planes.hip: byte planes of elements of 2, 4 or 8 bytes (n_elems > 0; every pointer and plane_stride 16-byte aligned).
// d_base (may be null) in every launch: the interleaved side is taken against it -- the planes of
// d_in ^ d_base, d_out = merge ^ d_base -- by the _delta kernels; null launches exactly the plain kernel
void launch_planes_split(const uint8_t* d_in, const uint8_t* d_base, uint64_t n_elems, uint32_t elem_bytes, uint8_t* d_planes,
                         uint64_t plane_stride, hipStream_t s);
// d_status (may be null): the launch stores nothing when the word is non-zero.  d_base == d_out is allowed
void launch_planes_merge(const uint8_t* d_planes, uint64_t plane_stride, const uint8_t* d_base, uint64_t n_elems, uint32_t elem_bytes,
                         uint8_t* d_out, const int* d_status, hipStream_t s);
// elements [first, first + count) of the planes (count > 0); reads [first & ~15, (first + count + 15) & ~15) of every plane
// and d_base[0 .. count * elem_bytes), the base of the range itself
void launch_planes_merge_range(const uint8_t* d_planes, uint64_t plane_stride, const uint8_t* d_base, uint64_t first, uint64_t count,
                               uint32_t elem_bytes, uint8_t* d_out, const int* d_status, hipStream_t s);
// the same with one device address per plane, read from a HOST array of elem_bytes entries.
// split_to: every h_dst[b] 16-byte aligned.  merge_from: h_src[b] is plane b's byte of the first element and all elem_bytes
// addresses are equal mod 16; that remainder is the skew (0: the unskewed kernel), and [h_src[b] & ~15, (h_src[b] + n_elems
// + 15) & ~15) of every plane is read.  d_base, d_status: as above
void launch_planes_split_to(const uint8_t* d_in, const uint8_t* d_base, uint64_t n_elems, uint32_t elem_bytes, uint8_t* const* h_dst,
                            hipStream_t s);
void launch_planes_merge_from(const uint8_t* const* h_src, const uint8_t* d_base, uint64_t n_elems, uint32_t elem_bytes, uint8_t* d_out,
                              const int* d_status, hipStream_t s);
// ghf_sparse.hip: n > 0, d_in / d_mask / d_vals / d_out 16-byte aligned.  d_counts: kSparseGroups words, d_offs: kSparseOffWords
// words, both private to the three launches each call queues (count, scan, move).
// split: mask[0 .. (n + 7) / 8) and *d_n_vals are always written; n_vals > vals_cap latches GHF_E_CAP and d_vals stays untouched
void launch_sparse_split(const uint8_t* d_in, uint64_t n, uint8_t* d_mask, uint8_t* d_vals, uint64_t vals_cap, uint64_t* d_n_vals,
                         uint64_t* d_counts, uint64_t* d_offs, int* d_status, hipStream_t s);
// merge: nothing is stored when *d_status is non-zero; set bits other than n_vals, or a set pad bit, latch GHF_E_CORRUPT
void launch_sparse_merge(const uint8_t* d_mask, const uint8_t* d_vals, uint64_t n_vals, uint64_t n, uint8_t* d_out, uint64_t* d_counts,
                         uint64_t* d_offs, int* d_status, hipStream_t s);
// the same with the values at d_vals[vals_skip .. vals_skip + n_vals): d_vals 16-byte aligned, vals_skip arbitrary
void launch_sparse_merge_at(const uint8_t* d_mask, const uint8_t* d_vals, uint64_t vals_skip, uint64_t n_vals, uint64_t n, uint8_t* d_out,
                            uint64_t* d_counts, uint64_t* d_offs, int* d_status, hipStream_t s);
// mask of a string of n bytes -> its rank table at d_table (16-byte aligned, kSparseRankHeaderBytes + 8 * (blocks + 1) bytes);
// three launches (count, scan, write); a set pad bit latches GHF_E_CORRUPT; nothing is stored behind a latched status
void launch_sparse_rank_pack(const uint8_t* d_mask, uint64_t n, uint8_t* d_table, uint64_t* d_counts, uint64_t* d_offs, int* d_status,
                             hipStream_t s);
// ghf_planes_hist.hip: elem_bytes is 2, 4 or 8, n_elems > 0, d_in 16-byte aligned.  d_acc: kPlanesHistAccWords words, zero
// between launches.  Two launches: the counting kernel, then the finish (replica sums, slot 256, GHF_HIST_COVER_ALL), which
// is also what zeroes d_acc again.  -> the first launch error; after an error of the finish launch d_acc is the caller's to clear.
// d_base (may be null, else 16-byte aligned): the counts are those of d_in ^ d_base
hipError_t launch_histogram_planes(const uint8_t* d_in, const uint8_t* d_base, uint64_t n_elems, uint32_t elem_bytes, uint32_t flags,
                                   uint64_t* d_acc, uint64_t* d_hists, hipStream_t s);
// d_bytes[p] <- image size of counts d_hists[p] under d_codes[p]; 0: the code is not complete or misses a counted byte
void launch_planes_image_bytes(const uint64_t* d_hists, const ghf_code* d_codes, uint32_t elem_bytes, uint64_t* d_bytes, hipStream_t s);
// latches GHF_E_FORMAT (a code is not a complete prefix code) or GHF_E_NOCODE (a counted byte has no code) at *d_status
void launch_planes_vet_codes(const uint64_t* d_hists, const ghf_code* d_codes, uint32_t elem_bytes, int* d_status, hipStream_t s);

// ghf_planes_gather.hip: rows [index[r] * index_stride, + row_elems) of a tensor of n_elems elements
// stored as elem_bytes planes, each a .crs2 image with a seek table or raw -> out + r * out_stride; row_status[r] <- the row's
// verdict.  Entry p of the arrays is plane p's; a raw plane's stream is the plane and its records and code are not read.
struct PlanesGatherParams {
  const uint8_t* streams[GHF_PLANES_MAX];  // 16-byte aligned
  uint64_t stream_bytes[GHF_PLANES_MAX];
  const uint8_t* records[GHF_PLANES_MAX];  // the seek table behind its header: n_blocks records
  const ghf_code* codes;                   // [elem_bytes]
  uint64_t n_elems, n_blocks;              // n_blocks = blocks_for(n_elems), what every table was held against
  const uint64_t* index;                   // [n_rows]
  uint64_t index_stride;
  uint32_t row_elems, n_rows;              // 1 <= row_elems <= GHF_GATHER_MAX_ROW_ELEMS
  uint32_t stage_bytes;                    // the launch's dynamic LDS: filled in by the launcher from row_elems
  uint8_t* out;
  uint64_t out_stride;                     // >= row_elems * elem_bytes
  int32_t* row_status;                     // [n_rows]
};
// one launch whatever n_rows is (none when it is 0); raw_planes has bits below elem_bytes only
void launch_decode_planes_gather(const PlanesGatherParams& p, uint32_t elem_bytes, uint32_t raw_planes, hipStream_t s);

// ghf_planes_gather_forms.hip: the same rows of a tensor stored in any mix of the three forms, against a
// base tensor where there is one.  The arrays have an entry per SLOT (the slot rule of section 20): j < elem_bytes is plane j's
// stream -- the plane itself, its .crs2 image, or the image of its mask -- and elem_bytes + p the image of sparse plane p's
// values, which is not read when n_vals[p] == 0.  A stored stream that has a code has its records; a raw plane's are not read.
struct PlanesGatherFormsParams {
  const uint8_t* streams[2 * GHF_PLANES_MAX];  // 16-byte aligned
  uint64_t stream_bytes[2 * GHF_PLANES_MAX];
  const uint8_t* records[2 * GHF_PLANES_MAX];  // the seek table behind its header: blocks_for(the slot's symbols) records
  const uint64_t* cum[GHF_PLANES_MAX];         // sparse plane p: cum[0 .. rank blocks] of its rank table image; untrusted
  uint64_t n_vals[GHF_PLANES_MAX];             // sparse plane p: what its rank info counts (<= n_elems), the symbols of slot E + p
  const ghf_code* codes;                       // [2 * elem_bytes]
  const uint8_t* base;                         // the whole base tensor, or null
  uint64_t n_elems;
  const uint64_t* index;                       // [n_rows]
  uint64_t index_stride;
  uint32_t row_elems, n_rows;                  // 1 <= row_elems <= the cap of the launch's forms
  uint32_t stage_bytes;                        // the launch's dynamic LDS ...
  uint32_t once;                               // ... which holds every plane of a row at once, or one plane: by the launcher
  uint8_t* out;
  uint64_t out_stride;                         // >= row_elems * elem_bytes
  int32_t* row_status;                         // [n_rows]
};
// one launch whatever n_rows is (none when it is 0); the masks have bits below elem_bytes only and share none
void launch_decode_planes_gather_forms(const PlanesGatherFormsParams& p, uint32_t elem_bytes, uint32_t raw_planes, uint32_t sparse_planes,
                                       hipStream_t s);

// ghf_tensor.hip: the container GHFTENS1 of one typed tensor.  A 768-byte head -- 128 bytes of fields,
// then a directory of 40 {u64 offset, u64 bytes}: entries 0 .. 15 the stored streams by slot, 16 .. 31 their seek tables, 32 .. 39
// the rank tables by plane -- and behind it the seek tables, the rank tables and the streams, each section 16-byte aligned and
// zero-padded to the next.  The tables' sizes are the host's, the streams' only the device's.
constexpr uint32_t kTensorHeadBytes = GHF_TENSOR_HEAD_BYTES;
constexpr uint32_t kTensorSlots = 2 * GHF_PLANES_MAX;
constexpr uint32_t kTensorFixed = kTensorSlots + GHF_PLANES_MAX;  // the directory entries whose sizes the host knows
constexpr uint64_t kTensorMagic = 0x31534E4554464847ull;          // "GHFTENS1"
constexpr uint32_t kTensorVersion = 1;
constexpr uint32_t kTensorPackGroups = 4096;  // the most slabs of the copy: 16 workgroups of 4 waves per CU, as k_stream_copy
struct TensorPackParams {
  const uint8_t* streams[kTensorSlots];  // slot j where it lies now (16-byte aligned, readable to its size rounded up to 16)
  const uint64_t* stream_bytes;          // DEVICE [2 * elem_bytes]: the streams' sizes
  uint32_t stored;                       // bit j: slot j holds a stream
  uint32_t elem_bytes, raw_planes, sparse_planes, flags;
  uint64_t n_elems;
  uint64_t n_vals[GHF_PLANES_MAX];       // as the head states them: 0 for a plane that is not sparse
  uint64_t fixed_off[kTensorFixed], fixed_bytes[kTensorFixed];  // directory entries 16 .. 39 ({0, 0}: absent); bytes % 8 == 0
  uint64_t streams_off;                  // where the stream region begins: the end of the host-known part
  uint8_t* out;                          // the container, 16-byte aligned
  uint64_t cap;
  uint64_t* out_bytes;                   // <- total_bytes, also when it exceeds cap
  int* status;
};
// one launch of `groups` workgroups (1 .. kTensorPackGroups); no workgroup waits for another
void launch_tensor_pack(const TensorPackParams& p, uint32_t groups, hipStream_t s);
// one workgroup per stored stream that has a code: every offset + bytes lies inside the container (the host's parse)
struct TensorOpenParams {
  const uint8_t* container;
  uint32_t n_streams;
  uint32_t slot[kTensorSlots];  // workgroup b vets the stream of slot[b] and fills codes[slot[b]]
  uint64_t stream_off[kTensorSlots], stream_bytes[kTensorSlots];
  uint64_t table_off[kTensorSlots], symbols[kTensorSlots];  // its seek table and the symbols the head gives the stream
  uint64_t rank_off[kTensorSlots], rank_n_vals[kTensorSlots];  // a mask's workgroup: its plane's rank table (0: none)
  uint64_t n_elems;
  ghf_code* codes;  // [2 * elem_bytes], all zero when the kernel starts
  int* status;
};
void launch_tensor_open(const TensorOpenParams& p, hipStream_t s);  // nothing is queued when n_streams == 0
// *d_dst <- value, unless *d_status is non-zero
void launch_tensor_store_size(uint64_t* d_dst, uint64_t value, const int* d_status, hipStream_t s);

}  // namespace ghf
#endif
