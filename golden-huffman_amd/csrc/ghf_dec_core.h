// golden-huffman_amd/csrc/ghf_dec_core.h -- what the decoders share: the table entry format and the replica rule, the
// tables in LDS, the miss path, the bit window and the padded input tiles.  Included by the decoder translation units only
// (ghf_decode.hip: table kernels + K7, ghf_sync.hip: K6, ghf_seek.hip: seek table + range head).
#ifndef GHF_DEC_CORE_H_
#define GHF_DEC_CORE_H_
#include "ghf_device.h"

namespace ghf {

// ---- entries ------------------------------------------------------------------------------------------------------
//   entry = symbol | length << 8 | bit 16: end mark | bit 17: no code of <= lut_bits bits starts with these bits
constexpr uint32_t kEntEnd = 1u << 16, kEntNone = 1u << 17;
__device__ __forceinline__ uint32_t dec7_entry(uint32_t g) {  // compact entry (sym | len << 9) -> image entry
  const uint32_t sym = g & 0x1FFu, len = g >> 9;
  return (sym & 0xFFu) | (len << 8) | (sym == 256u ? kEntEnd : 0u) | (len == 0u ? kEntNone : 0u);
}
// sym | len << 16, as the miss path finds it -> entry (sym 256: the end mark)
__device__ __forceinline__ uint32_t dec_long_to_entry(uint32_t r) { return (r & 0xFFu) | ((r >> 16) << 8) | ((r & 0x100u) << 8); }

// ---- the replica rule ---------------------------------------------------------------------------------------------
// K7 keeps the direct table in LDS as 32-bit entries, REPLICATED so that the 64 random lookups of a wave do not pile
// up on a few banks: the table gets 64 KiB = 16384 slots; with lut_bits index bits there is room for
// R = min(32, 2^(14 - lut_bits)) copies, slot = index * R + lane % R.  Up to 9-bit tables (uniform bytes: 8/9-bit codes)
// that is one bank per lane of a 32-lane LDS group: conflict-free whatever the data (PMC, 256 MiB uniform, round 1:
// 74 % of the LDS cycles of the 16-bit / 16-copy layout were bank-conflict cycles).  12-bit tables get 4 copies (skewed
// data hits few, mostly identical entries anyway: identical addresses broadcast).
// The room comes from the output: a lane keeps its 64 decoded bytes in 16 registers and the wave's INPUT tile, dead by
// then, serves as the transposition buffer for the coalesced copy-out.
// The table kernels (dec_image_fill) and every reader take log2(copies) of a table of `bits` index bits from here.  (A macro:
// as a function, __forceinline__ and constexpr included, it changes the code of k_build_decode_tables -- 33 -> 94 VGPRs.)
constexpr int kDecCopyShiftMax = 5;  // 32 copies; the small one-symbol table of pair mode (kDec7SmallSlots) always has them
#define GHF_DEC_COPY_SHIFT(bits) ((kDec7LutLog2 - (bits)) < kDecCopyShiftMax ? (kDec7LutLog2 - (bits)) : kDecCopyShiftMax)
// what a lane needs to look codes up in ITS replica of a table
struct DecLut {
  const char* base;  // table + 4 * (lane % copies)
  int lsh;           // 32 - index bits
  int ash;           // log2(copies) + 2
};
__device__ __forceinline__ uint32_t dec_lookup(const DecLut& T, uint32_t v) {
  return *reinterpret_cast<const uint32_t*>(T.base + ((v >> T.lsh) << T.ash));
}
// `shift` = log2(copies) of `table`
__device__ __forceinline__ DecLut dec_replica(const uint32_t* table, int bits, int shift, int lane) {
  DecLut T;
  T.base = reinterpret_cast<const char*>(table + ((uint32_t)lane & ((1u << shift) - 1u)));
  T.lsh = 32 - bits;
  T.ash = shift + 2;
  return T;
}
// a lane's replicas of the tables of an image (DecTables::image as copied into LDS): T1 = one symbol per lookup (behind the
// pair table, in 32 copies, when there is one), T2 = two (small alphabets only: pair_bits != 0)
__device__ __forceinline__ DecLut dec_lut1(const uint32_t* image, int lut_bits, int pair_bits, int lane) {
  return dec_replica(image + (pair_bits ? kDec7LutSlots : 0), lut_bits, pair_bits ? kDecCopyShiftMax : GHF_DEC_COPY_SHIFT(lut_bits), lane);
}
__device__ __forceinline__ DecLut dec_lut2(const uint32_t* image, int pair_bits, int lane) {
  return dec_replica(image, pair_bits, GHF_DEC_COPY_SHIFT(pair_bits), lane);
}

// ---- the padded input tiles (K7, K6) --------------------------------------------------------------------------------
constexpr int kDec7Threads = 1024;
constexpr int kDec7Waves = kDec7Threads / kWave;
constexpr int kDec7InBytes = 4608;  // staged span per wave: 4096 symbols at <= 9 bits average (a byte-Huffman code averages <= 8.1)
constexpr int kDec7InWords = kDec7InBytes / 4;
// The input tiles are PADDED: 16 bytes after every 128.  A lane's segment of uniform bytes is ~64 bytes long, so the 32
// lanes of an LDS group read "their current word" 16 words apart -- two banks for 32 lanes, a 16-way conflict on every
// window refill (PMC, round 2: 68 % of this kernel's LDS cycles).  With the pad, lanes two apart shift by four banks and
// only lanes l, l + 16 still share one (2-way: free).  All tiles live in one logical byte space (tile stride a multiple
// of 128) so that logical -> physical is two VALU instructions, no per-wave base: phys = la + (la >> 7 << 4).
constexpr int kDec7TileLog = kDec7InBytes + 128;                  // logical bytes per wave (16 zero bytes + slack behind the span)
constexpr int kDec7TilePhys = kDec7TileLog / 128 * 144;           // 5328
static_assert(kDec7TileLog % 128 == 0 && kDec7TilePhys >= 4096 + 16, "tile doubles as the 4 KiB transposition buffer");
__device__ __forceinline__ uint32_t in_phys(uint32_t la) {
  // two instructions, v_lshrrev + v_lshl_add (left to itself the compiler canonicalises (la >> 7) << 4 into shift, mask, add:
  // three -- and this sits in every window refill of every decoder)
  uint32_t t = la >> 7;
  asm("" : "+v"(t));
  return (t << 4) + la;
}
// big-endian word at logical byte address la of the padded input tiles
__device__ __forceinline__ uint32_t in_word(const uint8_t* lin, uint32_t la) { return *reinterpret_cast<const uint32_t*>(lin + in_phys(la)); }

// ---- the tables in LDS ----------------------------------------------------------------------------------------------
// What a replicated-table decoder keeps in LDS: the table image and the small tables.  70 KiB: on its own (the seek kernels --
// every lane reads its own stretch of the stream) two workgroups of 16 waves per CU, eight waves per SIMD.
struct DecLds {
  alignas(16) uint32_t lut[kDec7LutSlots + kDec7SmallSlots];
  uint32_t fcl[36];
  uint32_t sp[36];
  uint16_t symbol[GHF_NSYM + 3];
  uint16_t tl[256], tr[256];  // kind 1 (.crs): the tree
  uint32_t root;
  int kind;
  int status0;
};
static_assert(sizeof(DecLds) <= 80 * 1024, "two workgroups per CU");
// K7 / K6: the tables behind the waves' padded input tiles
struct DecLds7 {
  alignas(128) uint8_t in[kDec7Waves * kDec7TilePhys];  // compressed spans of the waves' groups, big-endian words, padded; then their output
  DecLds t;
};
static_assert(sizeof(DecLds7) <= 160 * 1024, "one workgroup of 16 waves per CU");
// (a function of its own: written into dec_lds_load the compiler orders two pairs of LDS stores of k_decode the other way round)
__device__ __forceinline__ void dec_small_load(DecLds& L, const DecTables* dt, int tid, int nthreads) {
  if (tid < 36) {
    L.fcl[tid] = dt->fc_left[tid];
    L.sp[tid] = dt->start_pos[tid];
  }
  for (int i = tid; i < GHF_NSYM; i += nthreads) L.symbol[i] = dt->symbol[i];
  for (int i = tid; i < 256; i += nthreads) {
    L.tl[i] = dt->tl[i];
    L.tr[i] = dt->tr[i];
  }
  if (tid == 0) {
    L.kind = dt->kind;
    L.root = dt->root;
  }
}
// the table image (DecTables::image, written by the table kernels in its final layout) and the small tables into LDS
__device__ __forceinline__ void dec_lds_load(DecLds& L, const DecTables* dt, int tid, int nthreads) {
  constexpr int kVecs = (kDec7LutSlots + kDec7SmallSlots) / 4;
  const uint4* const img4 = reinterpret_cast<const uint4*>(dt->image);
  uint4* const lut4 = reinterpret_cast<uint4*>(L.lut);
  for (int g = tid; g < kVecs; g += nthreads) lut4[g] = img4[g];
  dec_small_load(L, dt, tid, nthreads);
}

// ---- the bit window -------------------------------------------------------------------------------------------------
// A decoder's window over the stream is {W, nextw, o}: W holds 64 stream bits, `o` of them (from the top) already consumed,
// nextw the 32 bits behind W; one symbol costs a 64-bit shift, the table lookup and an add.  Where the words come from is
// the owner's business -- a padded LDS tile (K7, K6), unstaged global bytes (K7's cold path), prefetched global vectors
// (the seek kernels) -- so these take and give words, and the owner fetches:
//   W = win_open(w0, w1); nextw = w2;                      open at bit o < 32 of w0
//   if (o >= 32u) { win_shift(W, nextw, o); nextw = <the next word>; }
__device__ __forceinline__ uint64_t win_open(uint32_t w0, uint32_t w1) { return ((uint64_t)w0 << 32) | w1; }
__device__ __forceinline__ void win_shift(uint64_t& W, uint32_t nextw, uint32_t& o) {  // o >= 32: drop a consumed word
  W = (W << 32) | nextw;
  o -= 32u;
}
__device__ __forceinline__ uint32_t win_peek(uint64_t W, uint32_t o) { return (uint32_t)((W << o) >> 32); }  // the next 32 bits (o <= 32)
// the next 64 bits (o < 32)
__device__ __forceinline__ uint64_t win_peek64(uint64_t W, uint32_t nextw, uint32_t o) {
  return o ? ((W << o) | ((uint64_t)nextw >> (32u - o))) : W;
}

// ---- the miss path ----------------------------------------------------------------------------------------------------
// codes longer than the direct table: the reference's linear extension (canonical_huff_encoder.cc:554-557).
// returns sym | len << 16
__device__ __forceinline__ uint32_t dec_long(const DecLds& L, uint32_t hi, int lut_bits, int max_len) {
  if (L.kind == 1) {  // .crs: walk the tree from the root (huff_tree.cc:255-271); malformed trees end in "no symbol"
    uint32_t node = L.root;
    for (int l = 1; l <= max_len && l <= 32; ++l) {
      const uint32_t p = node - 256u;
      if (p >= 256u) break;
      node = ((hi >> (32 - l)) & 1u) ? L.tr[p] : L.tl[p];
      if (node < 256u) return node | ((uint32_t)l << 16);
    }
    return 256u | ((uint32_t)max_len << 16);
  }
  int l = lut_bits + 1;
  if (l > max_len) return 256u | ((uint32_t)max_len << 16);  // an incomplete table (bits no code starts with): no symbol
  while (l < max_len && hi < L.fcl[l]) ++l;
  const uint32_t k = L.sp[l] + ((hi - L.fcl[l]) >> (32 - l));
  return (k < GHF_NSYM ? (uint32_t)L.symbol[k] : 256u) | ((uint32_t)l << 16);
}
// the same walk over 64 stream bits: a .crs tree deeper than 32 (include/huff_tree.cc:157-170 keeps codes as strings; such a
// tree needs more than 3.5 million input bytes).  The callers' windows hold at least 65 bits behind the cursor.
__device__ __forceinline__ uint32_t dec_long64(const DecLds& L, uint64_t hi, int max_len) {
  uint32_t node = L.root;
  for (int l = 1; l <= max_len; ++l) {
    const uint32_t p = node - 256u;
    if (p >= 256u) break;
    node = ((hi >> (64 - l)) & 1ull) ? L.tr[p] : L.tl[p];
    if (node < 256u) return node | ((uint32_t)l << 16);
  }
  return 256u | ((uint32_t)max_len << 16);
}
__device__ __forceinline__ uint32_t dec_long_entry(const DecLds& L, uint32_t v, int lut_bits, int max_len) {
  return dec_long_to_entry(dec_long(L, v, lut_bits, max_len));
}
// ... for a window whose code may be longer than 32 bits (o < 32: the refill in front of every lookup guarantees it)
__device__ __forceinline__ uint32_t dec_long_entry_at(const DecLds& L, uint64_t W, uint32_t nextw, uint32_t o, int lut_bits, int max_len) {
  if (max_len <= 32) return dec_long_entry(L, win_peek(W, o), lut_bits, max_len);
  return dec_long_to_entry(dec_long64(L, win_peek64(W, nextw, o), max_len));
}

}  // namespace ghf
#endif
