// golden-huffman_amd/csrc/ghf_sync.hip -- K6: side-car reconstruction for streams that come without one, gfx950 / wave64.
// File:line citations are relative to the reference tree.
#include "ghf_dec_core.h"

namespace ghf {

// ------------------------------------------------------------------------------------------------
// K6: rebuild the side-car of a FOREIGN stream (a .crs2 written by the reference has no sync points).
// Huffman codes self-synchronise: a decoder started at a wrong bit falls into step with the true
// code boundaries after a few symbols.  The body is cut into 512-bit subsequences; every thread decodes
// its subsequence from its current guess of the first code boundary and tells its right neighbour where
// it landed.  Thread 0 starts at a true boundary, so the fixed point of this iteration is the true
// segmentation; passes repeat (only threads whose guess changed redo work) until nothing changes.
// Then symbol counts are prefix-summed, the end mark fixes n, and one more pass writes the bit position
// of every 64th symbol -- the same side-car K5 emits.
// All K6 kernels run on K7's engine: one 16-wave workgroup per CU, the 64 KiB replicated direct table
// (conflict-free lookups), padded input tiles (conflict-free window refills); a wave trip = 64
// subsequences = 4 KiB of stream.
// ------------------------------------------------------------------------------------------------
constexpr int kSubBits = 512;

// what K6Cursor::step2 needs of a canonical code with at most two lengths (k6_two)
struct K6Two {
  uint32_t thr;      // first code of the shorter length, left-justified (0: one length only)
  uint32_t lmin;     // the shorter length
  uint32_t eof_lo;   // the end mark's code, left-justified ...
  uint32_t eof_span; // ... and 2^(32 - its length): v - eof_lo < eof_span  <=>  the next code IS the end mark
};
// a lane's decode cursor over its wave's staged tile: 64-bit window + one word of look-ahead
struct K6Cursor {
  uint32_t la;  // logical byte address of the next word to fetch
  uint64_t W;
  uint32_t nextw, o;
  __device__ __forceinline__ void open(const uint8_t* lin, uint32_t la0, uint32_t pos) {
    la = la0 + ((pos >> 5) << 2);
    o = pos & 31u;
    W = win_open(in_word(lin, la), in_word(lin, la + 4u));
    nextw = in_word(lin, la + 8u);
    la += 12u;
  }
  __device__ __forceinline__ void refill(const uint8_t* lin) {
    if (o >= 32u) {
      win_shift(W, nextw, o);
      nextw = in_word(lin, la);
      la += 4u;
    }
  }
  // the entry (symbol | length << 8 | flags) of the code at the cursor; the cursor moves behind it.
  // lut_bits < 0: the caller knows that the direct table resolves every code (max_len <= 12, canonical): no miss path
  __device__ __forceinline__ uint32_t step(const uint8_t* lin, const DecLds& L, const DecLut& T, int lut_bits, int max_len) {
    refill(lin);
    if (lut_bits >= 0 && o >= 32u) refill(lin);  // (a code beyond 32 bits: two words.  Without the test repeated here the big kernels' listings change)
    const uint32_t v = win_peek(W, o);
    uint32_t ent = dec_lookup(T, v);
    if (lut_bits >= 0 && (ent & kEntNone)) ent = dec_long_entry_at(L, W, nextw, o, lut_bits, max_len);
    o += (ent >> 8) & 0xFFu;
    return ent;
  }
  // the same for a canonical code with at most TWO lengths (uniform bytes: 8 / 9 bits; 16 symbols: 4 / 5): which of the two a
  // code has is one comparison of the next bits with the first code of the shorter length -- no table, no LDS round trip
  // in the dependency chain (canonical_huff_encoder.cc:446-450: the first length whose left-justified first code is <= v).
  // Returns length << 8 (| kEntEnd for the end mark): all that K6 ever asks of an entry.
  __device__ __forceinline__ uint32_t step2(const uint8_t* lin, const K6Two& C) {
    refill(lin);
    const uint32_t v = win_peek(W, o);
    const uint32_t len = C.lmin + (v < C.thr ? 1u : 0u);
    o += len;
    return (len << 8) | ((v - C.eof_lo < C.eof_span) ? kEntEnd : 0u);
  }
};
// MODE 0: table + tree walk / linear extension, 1: the table resolves every code, 2: two lengths
template <int MODE>
__device__ __forceinline__ uint32_t k6_step(K6Cursor& c, const uint8_t* lin, const DecLds& L, const DecLut& T, int lut_bits, int max_len,
                                            const K6Two& C2) {
  if (MODE == 2) return c.step2(lin, C2);
  return c.step(lin, L, T, MODE == 1 ? -1 : lut_bits, max_len);
}

// Two codes of at most 16 bits behind ONE refill check (table + miss path, or table only): their entries; the window may
// move, the position (o) does not -- the caller commits one or both.  Half the refill / bounds / end-mark tests of two
// single steps: the generic K6 loops run at 2.3x K7's time per decoded symbol, and most of that is tests, not lookups.
template <int MODE>
__device__ __forceinline__ void k6_peek2(K6Cursor& c, const uint8_t* lin, const DecLds& L, const DecLut& T, int lut_bits, int max_len,
                                         uint32_t& e0, uint32_t& e1) {
  static_assert(MODE == 0 || MODE == 1, "two-length codes step by comparison");
  c.refill(lin);
  const uint32_t v0 = win_peek(c.W, c.o);
  e0 = dec_lookup(T, v0);
  if (MODE == 0 && (e0 & kEntNone)) e0 = dec_long_entry(L, v0, lut_bits, max_len);
  const uint32_t v1 = win_peek(c.W, c.o + ((e0 >> 8) & 0xFFu));  // (o < 32, a code <= 16 bits: >= 16 valid bits)
  e1 = dec_lookup(T, v1);
  if (MODE == 0 && (e1 & kEntNone)) e1 = dec_long_entry(L, v1, lut_bits, max_len);
}

// stage the bits of 64 consecutive subsequences (+ look-ahead) of the body into the wave's padded tile (big-endian
// words, zeros behind the stream); returns the bit offset of subsequence `sub0` inside the tile
__device__ __forceinline__ uint32_t k6_stage(const SyncParams& P, uint64_t sub0, uint8_t* lin, uint32_t la0, int lane) {
  const uint64_t bit0 = P.body_bit0 + sub0 * kSubBits;
  const uint64_t byte0 = (bit0 >> 3) & ~15ull;
  uint64_t byte1 = ((bit0 + 64ull * kSubBits + 7) >> 3) + 32;  // look-ahead: a code of <= 64 bits that begins in the last subsequence + the cursor's three words
  if (byte1 > P.stream_bytes) byte1 = P.stream_bytes;
  const uint32_t span = byte1 > byte0 ? (uint32_t)(byte1 - byte0) : 0u;
  const uint8_t* src = P.stream + byte0;
#pragma unroll
  for (int k = 0; k < (kDec7TileLog + 1023) / 1024; ++k) {
    const uint32_t o = (uint32_t)k * 1024u + (uint32_t)lane * 16u;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (o + 16u <= span) {
      v = *reinterpret_cast<const uint4*>(src + o);
    } else if (o < span) {  // the stream's last, incomplete 16 bytes: byte loads, never past the end of the buffer
      uint32_t q[4] = {0, 0, 0, 0};
      for (uint32_t j = 0; o + j < span; ++j) q[j >> 2] |= (uint32_t)src[o + j] << (8 * (j & 3));
      v = make_uint4(q[0], q[1], q[2], q[3]);
    }
    if (o + 16u <= (uint32_t)kDec7TileLog)
      *reinterpret_cast<uint4*>(lin + in_phys(la0 + o)) = make_uint4(bswap32(v.x), bswap32(v.y), bswap32(v.z), bswap32(v.w));
  }
  return (uint32_t)(bit0 - byte0 * 8);
}

// the two-length facts of a canonical code (meaningless, and unused, for any other code): from the tables in LDS
__device__ __forceinline__ K6Two k6_two(const DecLds& L, int min_len, int max_len) {
  K6Two C;
  C.lmin = (uint32_t)min_len;
  C.thr = max_len > min_len ? L.fcl[min_len & 31] : 0u;
  // the end mark is the largest symbol, hence the LAST code of its length: it sits at the end of its length's run in symbol[]
  int k = 0;
  while (k < GHF_NSYM && L.symbol[k] != 256) ++k;
  const int len = (max_len > min_len && k >= (int)L.sp[max_len & 31]) ? max_len : min_len;
  const uint32_t code_left = L.fcl[len & 31] + (((uint32_t)k - L.sp[len & 31]) << ((32 - len) & 31));
  C.eof_lo = k < GHF_NSYM ? code_left : 0xFFFFFFFFu;
  C.eof_span = k < GHF_NSYM ? (1u << ((32 - len) & 31)) : 0u;
  return C;
}

constexpr int kK6Threads = kDec7Threads;
constexpr int kK6Waves = kDec7Waves;

// what every K6 kernel starts with: tables into LDS, this lane's table replica, the wave's tile
#define GHF_K6_PROLOGUE()                                                  \
  __shared__ DecLds7 L;                                                    \
  const int tid = threadIdx.x;                                             \
  dec_lds_load(L.t, P.dt, tid, kK6Threads);                                \
  __syncthreads();                                                         \
  const int lane = tid & 63;                                               \
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);               \
  const int lut_bits = P.dt->lut_bits, max_len = P.dt->max_len;            \
  const bool direct = P.dt->kind == 0 && max_len <= kDecLutBitsMax;        \
  const int k6_mode = (P.dt->kind == 0 && max_len - P.dt->min_len <= 1 && max_len <= 31) ? 2 : (direct ? 1 : 0); \
  const K6Two C2 = k6_two(L.t, P.dt->min_len, max_len);                    \
  const DecLut T1 = dec_lut1(L.t.lut, P.dt->lut_bits, P.dt->pair_bits, lane); \
  uint8_t* const lin = L.in;                                               \
  const uint32_t la0 = (uint32_t)wave * kDec7TileLog;                      \
  const uint64_t ngroups = (P.nsub + 63) >> 6;                             \
  const uint64_t body_bits = P.end_bit - P.body_bit0

__device__ __forceinline__ uint32_t k6_limit(uint64_t body_bits, uint64_t g) {  // end of the stream, relative to the wave's first subsequence
  const uint64_t l = body_bits - g * 64 * kSubBits;
  return l > 0x7FFFFFFFull ? 0x7FFFFFFFu : (uint32_t)l;
}

// ---- classes: K6 on canonical codes of L and L + 1 bits, L = 8 or 4 ---------------------------------------------------
// Bytes that do not compress -- 256 byte values + the end mark, none of them rare enough for a 10-bit code: 255 codes of 8
// bits and two of 9 (the least frequent value and the end mark: 9-bit codes 0 and 1, every 8-bit code >= 0x01) -- and the
// same shape one size down, 16 equally likely values + the end mark: 15 codes of 4 bits, two of 5.  A decoder that stands at
// bit p moves to p + L, or to p + L + 1 when the L bits at p are zero.  So it walks along the positions of its CLASS p mod 8
// (L = 4: of the two classes p mod 8 and p + 4 mod 8, alternately) until it meets L zero bits, and then along the next
// class: per subsequence a handful of jumps instead of 57 (128) steps -- and max_len chains of them in k_sync_table: these
// codes are the ones that re-synchronise slowest.  The 64 positions of class r are one 64-bit mask F[r] (bit 63 - i: the
// L bits at bit 8 i + r are zero), computed for all eight classes at once from the bit planes of the subsequence's 64 bytes
// (8 x 8 bit-matrix transposes: no step touches a single symbol); G[r] marks those of them whose next bit makes the code
// the end mark.
struct K6Cls {
  int L;             // 8 or 4: the code is of that kind (wave-uniform); 0: it is not
  uint32_t eof_bit;  // last bit of the end mark's code
};
__device__ __forceinline__ K6Cls k6_cls(int k6_mode, int min_len, int max_len, const K6Two& C2, uint64_t body_bit0) {
  K6Cls B;
  // (a body begins on a 4-byte boundary of a 16-byte aligned buffer: behind a .crs2 header, or at byte 0 of a piece)
  const bool shape = k6_mode == 2 && max_len == min_len + 1 && (min_len == 8 || min_len == 4) && C2.thr == (1u << (32 - min_len)) &&
                     C2.eof_span == (1u << (31 - min_len)) && C2.eof_lo < C2.thr && (body_bit0 & 31u) == 0;
  B.L = shape ? min_len : 0;
  B.eof_bit = (C2.eof_lo >> ((31 - min_len) & 31)) & 1u;
  return B;
}
__device__ __forceinline__ uint32_t bfi32(uint32_t m, uint32_t a, uint32_t b) { return (m & a) | (~m & b); }  // v_bfi_b32
// exchange the bits under m with the bits under m << d
__device__ __forceinline__ uint32_t delta_swap32(uint32_t x, uint32_t m, int d) { return bfi32(m, x >> d, bfi32(m << d, x << d, x)); }

// F (and G) of the subsequence that begins at bit `bitpos` (a multiple of 32: k6_cls) of the wave's staged tile
template <int L, bool WITH_EOF>
__device__ __forceinline__ void k6_classes(const uint8_t* lin, uint32_t la0, uint32_t bitpos, uint32_t eof_bit, uint64_t (&F)[8], uint64_t (&G)[8]) {
  static_assert(L == 8 || L == 4, "class length");
  const uint32_t la = la0 + ((bitpos >> 5) << 2);
  uint32_t E[17];  // the subsequence's 512 bits + 32 of look-ahead, first bit in bit 31 of E[0]
#pragma unroll
  for (int k = 0; k < 17; ++k) E[k] = in_word(lin, la + 4u * (uint32_t)k);
  // transpose every group of 8 bytes (rows = bytes, first byte on top): T[g][0] holds bit planes 0..3 (plane s = bit s of
  // every byte, most significant first; byte 3 - s of the word), T[g][1] planes 4..7
  uint32_t T[8][2];
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    uint32_t hi = delta_swap32(delta_swap32(E[2 * g], 0x00AA00AAu, 7), 0x0000CCCCu, 14);
    uint32_t lo = delta_swap32(delta_swap32(E[2 * g + 1], 0x00AA00AAu, 7), 0x0000CCCCu, 14);
    T[g][0] = bfi32(0xF0F0F0F0u, hi, lo >> 4);
    T[g][1] = bfi32(0xF0F0F0F0u, hi << 4, lo);
  }
  // plane s of all 64 bytes: Q[s][0] = bytes 0..31, Q[s][1] = bytes 32..63 (byte i in bit 31 - i mod 32)
  constexpr int NQ = 8 + L + (WITH_EOF ? 0 : -1);  // planes 0 .. 7 + L (7 + L - 1 without the end-mark masks)
  uint32_t Q[16][2];
#pragma unroll
  for (int half = 0; half < 2; ++half) {
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const uint32_t a = T[4 * hh][half], b = T[4 * hh + 1][half], c = T[4 * hh + 2][half], d = T[4 * hh + 3][half];
      const uint32_t abx = __builtin_amdgcn_perm(a, b, 0x07030602u), aby = __builtin_amdgcn_perm(a, b, 0x05010400u);
      const uint32_t cdx = __builtin_amdgcn_perm(c, d, 0x07030602u), cdy = __builtin_amdgcn_perm(c, d, 0x05010400u);
      Q[4 * half + 0][hh] = __builtin_amdgcn_perm(abx, cdx, 0x07060302u);
      Q[4 * half + 1][hh] = __builtin_amdgcn_perm(abx, cdx, 0x05040100u);
      Q[4 * half + 2][hh] = __builtin_amdgcn_perm(aby, cdy, 0x07060302u);
      Q[4 * half + 3][hh] = __builtin_amdgcn_perm(aby, cdy, 0x05040100u);
    }
  }
  // planes 8..: the same bits one byte later (bit s of bytes 1..64)
#pragma unroll
  for (int s = 0; s + 8 < NQ; ++s) {
    Q[s + 8][0] = alignbit(Q[s][0], Q[s][1], 31);
    Q[s + 8][1] = (Q[s][1] << 1) | ((E[16] >> (31 - s)) & 1u);
  }
  const uint32_t eofx = eof_bit ? 0u : 0xFFFFFFFFu;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    uint32_t f[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      uint32_t any = Q[r][h] | Q[r + 1][h] | Q[r + 2][h] | Q[r + 3][h];
      if (L == 8) any |= Q[r + 4][h] | Q[r + 5][h] | Q[r + 6][h] | Q[r + 7][h];
      f[h] = ~any;
    }
    F[r] = ((uint64_t)f[0] << 32) | f[1];
    if (WITH_EOF) G[r] = ((uint64_t)(f[0] & (Q[r + L][0] ^ eofx)) << 32) | (f[1] & (Q[r + L][1] ^ eofx));
  }
}
// where the masks of a wave's 64 subsequences live while its chains walk: F in the (unused) table area, [class][thread];
// G in the wave's own tile, whose bytes are in registers by then, [class][lane]
// (the masks are 64-bit words in arrays that are declared, and elsewhere accessed, as 32-bit words and bytes: may_alias
//  tells the compiler so -- without it type-based alias analysis may order these accesses freely against the others)
typedef uint64_t __attribute__((may_alias)) k6_mask_t;
__device__ __forceinline__ k6_mask_t* k6_f_slot(DecLds7& L, int tid) { return reinterpret_cast<k6_mask_t*>(L.t.lut) + tid; }
__device__ __forceinline__ k6_mask_t* k6_g_slot(DecLds7& L, int wave, int lane) {
  return reinterpret_cast<k6_mask_t*>(L.in + (uint32_t)wave * kDec7TilePhys) + lane;
}
static_assert(sizeof(DecLds::lut) >= 8 * kDec7Threads * sizeof(uint64_t) && kDec7TilePhys >= 8 * 64 * (int)sizeof(uint64_t) && kDec7TilePhys % 8 == 0,
              "room for the class masks");
// One jump of a chain that stands at bit p < 512 of its subsequence: s = the L-bit codes in front of the next (L + 1)-bit
// code (found), or in front of the subsequence's end; eof = that code is the end mark.  fmask(c) / gmask(c) = the F / G mask
// of class c (from LDS; from registers when p is a compile-time constant).  All mask reads are issued together: a jump is
// ONE LDS round trip.
template <int L, bool WITH_G, typename FM, typename GM>
__device__ __forceinline__ uint32_t k6_jump(FM fmask, GM gmask, uint32_t p, bool& found, bool& eof) {
  const uint32_t a = p & 7u, i = p >> 3;
  if (L == 8) {
    const uint64_t m = fmask(a) << i;
    const uint64_t g = WITH_G ? gmask(a) << i : 0ull;
    found = m != 0;
    const uint32_t z = (uint32_t)__builtin_clzll(m | 1ull);
    eof = WITH_G && found && ((g << z) >> 63);
    return found ? z : 64u - i;
  }
  // L = 4: the chain alternates between class a (steps 0, 2, ..) and class a + 4 mod 8 (steps 1, 3, ..: the same byte when
  // a < 4, the next one otherwise)
  const uint32_t b = (a + 4u) & 7u, ib = i + (a >> 2), ibm = ib & 63u;
  const uint64_t ma = fmask(a) << i;
  const uint64_t mb = ib < 64u ? fmask(b) << ibm : 0ull;
  const uint64_t ga = WITH_G ? gmask(a) << i : 0ull;
  const uint64_t gb = WITH_G ? gmask(b) << ibm : 0ull;
  const uint32_t ta = (uint32_t)__builtin_clzll(ma | 1ull), tb = (uint32_t)__builtin_clzll(mb | 1ull);
  const uint32_t sa = ma ? 2u * ta : 1000u;
  const uint32_t sb = mb ? 2u * tb + 1u : 1000u;
  const bool first_a = sa < sb;
  const uint32_t s = first_a ? sa : sb;
  found = s < 1000u;
  eof = WITH_G && found && (((first_a ? ga << ta : gb << tb) >> 63) != 0);
  return found ? s : (515u - p) >> 2;
}

__global__ __launch_bounds__(kK6Threads, 4) void k_sync_pass(SyncParams P) {
  GHF_K6_PROLOGUE();
  auto run = [&](auto mode_tag) {
  constexpr int MODE = decltype(mode_tag)::value;
  for (uint64_t g = (uint64_t)blockIdx.x * kK6Waves + wave; g < ngroups; g += (uint64_t)gridDim.x * kK6Waves) {
    const uint64_t sub = g * 64 + lane;
    const bool valid = sub < P.nsub;
    uint32_t st = 0;
    bool work = false, moved = false;
    if (valid) {
      st = (P.first & 2u) ? (sub == 0 ? P.first_start : 0u) : P.start[sub];
      work = (P.first & 1u) ? true : P.used[sub] != st;
    }
    if (!__ballot(work)) continue;  // the whole wave's results are still current
    wave_sync();
    const uint32_t base = k6_stage(P, g * 64, lin, la0, lane);
    wave_sync();
    if (work) {
      const uint32_t sub_lo = (uint32_t)lane * kSubBits;  // relative to the wave's first subsequence
      const uint32_t sub_hi = sub_lo + kSubBits;
      const uint32_t limit = k6_limit(body_bits, g);
      const bool pairs = max_len <= 16 && limit >= 64u * kSubBits;  // (wave-uniform: short codes, every subsequence whole)
      uint32_t pos = sub_lo + st;
      uint32_t count = 0;
      bool eof = false;
      K6Cursor cur;
      cur.open(lin, la0, base + pos);
      if (MODE != 2 && pairs) {  // two codes per round while neither is an end mark; what is left goes one by one below
        while (pos < sub_hi) {
          uint32_t e0, e1;
          k6_peek2<MODE == 2 ? 1 : MODE>(cur, lin, L.t, T1, lut_bits, max_len, e0, e1);
          if ((e0 | e1) & kEntEnd) break;
          const uint32_t l0 = (e0 >> 8) & 0xFFu, l1 = (e1 >> 8) & 0xFFu;
          const bool both = pos + l0 < sub_hi;  // the second code begins in this subsequence too
          pos += both ? l0 + l1 : l0;
          cur.o += both ? l0 + l1 : l0;
          count += both ? 2u : 1u;
        }
      }
      while (pos < sub_hi && pos < limit) {
        const uint32_t ent = k6_step<MODE>(cur, lin, L.t, T1, lut_bits, max_len, C2);
        if (ent & kEntEnd) {  // the end mark (or bits that are no code)
          eof = true;
          break;
        }
        pos += (ent >> 8) & 0xFFu;
        ++count;
      }
      // .crs has no end mark: "eof" then means "this cannot be right" -- a bit pattern that is no code, or a last
      // code that runs past the end of the stream
      if (P.no_eof == 1u && pos > limit) eof = true;
      P.cnt[sub] = count;
      P.eof[sub] = eof ? 1 : 0;
      P.used[sub] = (uint16_t)st;
      if (P.first & 2u) {
        // the launch that fills `start`: every subsequence stores its neighbour's guess, 0 ("nothing known") included
        if (sub + 1 < P.nsub) {
          const uint16_t land = (!eof && pos >= sub_hi) ? (uint16_t)(pos - sub_hi) : (uint16_t)0;
          P.start[sub + 1] = land;
          if (land) {
            *P.changed = 1;
            moved = true;
          }
        } else if (P.no_eof != 2u) {
          P.start[P.nsub] = 0;  // (the landing slot: a piece's last subsequence stores it below)
        }
      } else if (!eof && pos >= sub_hi && sub + 1 < P.nsub) {
        const uint16_t land = (uint16_t)(pos - sub_hi);
        if (P.start[sub + 1] != land) {
          P.start[sub + 1] = land;
          *P.changed = 1;
          moved = true;
        }
      }
      // a PIECE of a stream (mode 2, multi-GPU decode): the last code may run into the next piece's bytes (they are
      // there as look-ahead); where it ends is the next piece's first code boundary
      if (P.no_eof == 2u && sub + 1 == P.nsub) P.start[P.nsub] = eof ? (uint16_t)0xFFFF : (uint16_t)(pos - limit);
    }
    // ... and roughly how MANY boundaries moved, for the driver's choice between more passes and the deterministic scan:
    // every 256th group adds its count to the word behind the flag (all groups would be three million atomics on one
    // address in a 4 GiB stream's first pass)
    const uint64_t mv = __ballot(moved);
    if (mv && lane == 0) {
      if ((g & 255u) == 0) atomicAdd(P.changed + 1, (uint32_t)__builtin_popcountll(mv));
      // ... and WHERE the first of them is: nothing in front of the stream's end mark moving any more is all the driver
      // needs (a buffer may go on behind its end mark -- stale bytes -- and those never have to settle).  Stored inverted
      // so that "none" is the zero the flag's memset leaves; the read in front keeps the atomics to the few that improve it
      const unsigned long long inv = ~(g * 64 + (uint64_t)__builtin_ctzll(mv));
      if (inv > __hip_atomic_load(P.moved_first_inv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(P.moved_first_inv, inv);
    }
  }
  };
  if (k6_mode == 2) run(std::integral_constant<int, 2>{});
  else if (k6_mode == 1) run(std::integral_constant<int, 1>{});
  else run(std::integral_constant<int, 0>{});
}

// ---- K6 for streams that do not self-synchronise quickly (near-fixed-length codes: uniform bytes have 8/9-bit codes and a
// decoder started at a wrong bit needs ~1000 symbols to fall into step, so the fixed-point passes above advance a few
// subsequences per launch).  Deterministic instead: for every subsequence the landing offset of EVERY possible start
// offset (a code straddles a boundary by less than max_len <= 32 bits) is one small function; where the true decode
// enters each subsequence is the running composition of those functions -- a parallel scan over function composition
// (64-ary tree: reduce up, apply down).  The result only seeds start[]: the fixed-point passes then verify it in one
// pass (and would repair it), so no format subtlety (end mark, end of a .crs, stream pieces) lives here.
// A function is STRIDE bytes (16 when max_len <= 16, 32 up to 32, else 64): entry s = landing offset in the next subsequence.
//
// k_sync_table: lane = subsequence, its max_len chains five at a time -- independent shift -> lookup -> add
// dependency chains per lane hide the LDS round trip that a single chain leaves exposed (four waves per SIMD do not).
//
// Classes (k6_classes, codes of L and L + 1 bits): the max_len chains of a subsequence are walks over the class masks -- per
// chain and round one or two LDS reads of the masks of its class, a shift, a count of leading zeros.  The row then also
// says, for every entry offset, how many (L + 1)-bit codes the chain met and whether one of them was the end mark: with the
// entry offset that the scan arrives at, that IS the subsequence's symbol count -- the lowest k_fn_apply settles every
// subsequence whose true chain met no end mark, and the confirming pass has only the others left.
//   row, L = 8: bytes 0..8 landing offsets | 10..11 end-mark bits | 12..15 nine 3-bit counts (7 = seven or more)
//   row, L = 4: bytes 0..4 landing offsets | 5..9 five 8-bit counts (255 = or more) | 10..11 end-mark bits
__global__ __launch_bounds__(kK6Threads, 4) void k_sync_table(SyncParams P, uint32_t stride, uint8_t* __restrict__ tab, uint32_t* __restrict__ cls_flag) {
  GHF_K6_PROLOGUE();
  const uint32_t S = (uint32_t)max_len < stride ? (uint32_t)max_len : stride;
  const K6Cls CL = k6_cls(k6_mode, P.dt->min_len, max_len, C2, P.body_bit0);
  if (blockIdx.x == 0 && tid == 0) *cls_flag = (uint32_t)CL.L;
  auto run = [&](auto mode_tag) {
  constexpr int MODE = decltype(mode_tag)::value;
  for (uint64_t g = (uint64_t)blockIdx.x * kK6Waves + wave; g < ngroups; g += (uint64_t)gridDim.x * kK6Waves) {
    wave_sync();
    const uint32_t base = k6_stage(P, g * 64, lin, la0, lane);
    wave_sync();
    const uint64_t sub = g * 64 + (uint64_t)lane;
    if (sub >= P.nsub) continue;
    const uint32_t limit = k6_limit(body_bits, g);
    const uint32_t lo = (uint32_t)lane * kSubBits;
    if (MODE == 2 && CL.L && limit >= 64u * kSubBits) {  // (wave-uniform: every lane's subsequence is whole)
      auto walk = [&](auto l_tag) {
        constexpr int CLEN = decltype(l_tag)::value, NCH = CLEN + 1;  // the chains: entry offsets 0 .. L
        uint64_t F[8], G[8];
        k6_classes<CLEN, true>(lin, la0, base + lo, CL.eof_bit, F, G);
        wave_sync();  // (every lane has its bytes: the tile may take the G masks)
        k6_mask_t* const Fl = k6_f_slot(L, tid);
        k6_mask_t* const Gl = k6_g_slot(L, wave, lane);
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          Fl[r * kK6Threads] = F[r];
          Gl[r * 64] = G[r];
        }
        // a chain = the bit p at which its next code begins; >= 512: it has left the subsequence
        uint32_t p[NCH], nl[NCH], eofs = 0;
        bool any = false;
#pragma unroll
        for (int e = 0; e < NCH; ++e) {  // first round: every chain stands at its entry offset, the masks still in registers
          bool found, eof;
          const uint32_t sh = k6_jump<CLEN, true>([&](uint32_t c) { return F[c]; }, [&](uint32_t c) { return G[c]; }, (uint32_t)e, found, eof);
          const uint32_t q = (uint32_t)e + (uint32_t)CLEN * sh;  // the long code (found), or the first position behind the subsequence
          p[e] = found ? q + (uint32_t)CLEN + 1u : q;
          nl[e] = found ? 1u : 0u;
          eofs |= eof ? (1u << e) : 0u;
          any |= p[e] < 512u;
        }
        while (any) {
          any = false;
#pragma unroll
          for (int e = 0; e < NCH; ++e) {
            const bool act = p[e] < 512u;
            const uint32_t pe = act ? p[e] : 0u;
            bool found, eof;
            // (L = 8: the long code lies in the chain's own class, its G mask is read WITH the F mask -- one LDS round trip per
            //  jump.  L = 4: it lies in one of two classes; reading both candidates' G masks up front gave wrong end-mark bits
            //  in THIS kernel at -O3 -- not at -O1, not with every s_waitcnt forced to zero (so it is not a counted wait), not
            //  in stand-alone GPU harnesses of the same function and loop, scratch/jump_gpu_test.hip / walk_gpu_test.hip, and
            //  not on the host -- which is not root-caused; that build is also the only one that spills (4 VGPRs).  The mask
            //  of the class the jump arrives in is read behind it, and tests/test_cabi_cpu.py keeps this kernel scratch-free.)
            const uint32_t sh = k6_jump<CLEN, CLEN == 8>([&](uint32_t c) { return Fl[c * kK6Threads]; }, [&](uint32_t c) { return Gl[c * 64]; }, pe, found, eof);
            const uint32_t q = pe + (uint32_t)CLEN * sh;
            if (CLEN == 4) eof = found && ((Gl[(q & 7u) * 64] << ((q >> 3) & 63u)) >> 63) != 0;
            p[e] = act ? (found ? q + (uint32_t)CLEN + 1u : q) : p[e];
            nl[e] += (act && found) ? 1u : 0u;
            eofs |= (act && eof) ? (1u << e) : 0u;
            any |= p[e] < 512u;
          }
        }
        uint4 row;
        if (CLEN == 8) {
          uint32_t w3 = 0;
#pragma unroll
          for (int e = 0; e < NCH; ++e) w3 |= (nl[e] < 7u ? nl[e] : 7u) << (3 * e);
          row = make_uint4((p[0] - 512u) | (p[1] - 512u) << 8 | (p[2] - 512u) << 16 | (p[3] - 512u) << 24,
                           (p[4] - 512u) | (p[NCH > 5 ? 5 : 0] - 512u) << 8 | (p[NCH > 6 ? 6 : 0] - 512u) << 16 | (p[NCH > 7 ? 7 : 0] - 512u) << 24,
                           (p[NCH > 8 ? 8 : 0] - 512u) | eofs << 16, w3);
        } else {
          uint32_t n[NCH];
#pragma unroll
          for (int e = 0; e < NCH; ++e) n[e] = nl[e] < 255u ? nl[e] : 255u;
          row = make_uint4((p[0] - 512u) | (p[1] - 512u) << 8 | (p[2] - 512u) << 16 | (p[3] - 512u) << 24,
                           (p[4] - 512u) | n[0] << 8 | n[1] << 16 | n[2] << 24, n[3] | n[4] << 8 | eofs << 16, 0u);
        }
        *reinterpret_cast<uint4*>(tab + sub * stride) = row;
      };
      if (CL.L == 8) walk(std::integral_constant<int, 8>{});
      else walk(std::integral_constant<int, 4>{});
      continue;
    }
    const uint32_t hi = lo + kSubBits < limit ? lo + kSubBits : limit;  // (behind the stream's end nothing is decoded)
    uint8_t* const row = tab + sub * stride;
    constexpr uint32_t NC = 5;  // chains in flight per lane
    const uint32_t nfree = limit >= 64u * kSubBits ? ((uint32_t)kSubBits - S) / (uint32_t)max_len : 0u;  // (wave-uniform: every lane's subsequence is whole)
    for (uint32_t s0 = 0; s0 < S; s0 += NC) {
      K6Cursor c[NC];
      uint32_t p[NC];
#pragma unroll
      for (uint32_t j = 0; j < NC; ++j) {
        p[j] = lo + s0 + j;
        c[j].open(lin, la0, base + p[j]);
        if (s0 + j >= S && nfree == 0u) p[j] = hi;  // no such chain (with free steps it simply runs along: never stored)
      }
      // the first (512 - S) / max_len steps cannot carry any chain out of its subsequence: no test per step (a chain
      // slot that stands for no entry offset steps along behind the subsequence -- inside the tile, never stored)
      for (uint32_t k = 0; k < nfree; ++k) {
#pragma unroll
        for (uint32_t j = 0; j < NC; ++j) p[j] += (k6_step<MODE>(c[j], lin, L.t, T1, lut_bits, max_len, C2) >> 8) & 0xFFu;
      }
      for (;;) {
        bool any = false;
#pragma unroll
        for (uint32_t j = 0; j < NC; ++j) {
          if (p[j] < hi) {
            p[j] += (k6_step<MODE>(c[j], lin, L.t, T1, lut_bits, max_len, C2) >> 8) & 0xFFu;
            any = true;
          }
        }
        if (!any) break;
      }
      const uint32_t end = lo + kSubBits;
#pragma unroll
      for (uint32_t j = 0; j < NC; ++j)
        if (s0 + j < S) row[s0 + j] = p[j] >= end ? (uint8_t)(p[j] - end) : (uint8_t)0;
    }
  }
  };
  if (k6_mode == 2) run(std::integral_constant<int, 2>{});
  else if (k6_mode == 1) run(std::integral_constant<int, 1>{});
  else run(std::integral_constant<int, 0>{});
}

// one level up: out[t] = f[64 t + 63] o ... o f[64 t]  (entry s: where a decode that enters tile t at offset s leaves it)
__global__ __launch_bounds__(64) void k_fn_reduce(const uint8_t* __restrict__ f, uint64_t n, uint32_t stride, uint8_t* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint8_t fl[64 * 64];
  const uint64_t t = blockIdx.x;
  const int lane = threadIdx.x;
  const uint64_t first = t * 64;
  const int cnt = (int)((n - first < 64) ? (n - first) : 64);
  for (int i = lane; i < cnt * (int)stride / 16; i += 64)
    reinterpret_cast<uint4*>(fl)[i] = reinterpret_cast<const uint4*>(f + first * stride)[i];
  __syncthreads();
  if (lane < (int)stride) {
    uint32_t cur = (uint32_t)lane;
    for (int j = 0; j < cnt; ++j) cur = fl[j * stride + (cur & (stride - 1))];
    out[t * stride + lane] = (uint8_t)cur;
  }
}

// one level down: start[64 t + j] = offset at which the true decode enters element j of tile t, given where it enters the
// tile.  The lowest level writes the subsequences' start offsets themselves (16-bit, P.start; [0] keeps the caller's value).
// With classes (*cls_flag = L, see k_sync_table) the lowest level also SETTLES the subsequences below n_settle: count and
// "computed from this entry offset" as k_sync_pass would leave them, unless the row says that the chain from this entry
// met an end mark or more 9-bit codes than the row counts.
template <typename OutT>
__global__ __launch_bounds__(64) void k_fn_apply(const uint8_t* __restrict__ f, uint64_t n, uint32_t stride,
                                                 const uint8_t* __restrict__ tile_start, uint32_t entry, OutT* __restrict__ start,
                                                 const uint32_t* __restrict__ cls_flag, uint64_t n_settle, uint32_t* __restrict__ cnt_out,
                                                 uint16_t* __restrict__ used_out, uint8_t* __restrict__ eof_out) {
  __shared__ __attribute__((aligned(16))) uint8_t fl[64 * 64];
  __shared__ uint8_t st[64];
  const uint64_t t = blockIdx.x;
  const int lane = threadIdx.x;
  const uint64_t first = t * 64;
  const int cnt = (int)((n - first < 64) ? (n - first) : 64);
  for (int i = lane; i < cnt * (int)stride / 16; i += 64)
    reinterpret_cast<uint4*>(fl)[i] = reinterpret_cast<const uint4*>(f + first * stride)[i];
  __syncthreads();
  if (lane == 0) {
    uint32_t cur = tile_start ? tile_start[t] : entry;  // top level: where the caller says the first code begins
    for (int j = 0; j < cnt; ++j) {
      st[j] = (uint8_t)cur;
      cur = fl[j * stride + (cur & (stride - 1))];
    }
  }
  __syncthreads();
  if (lane < cnt && (sizeof(OutT) == 1 || first + lane != 0)) start[first + lane] = (OutT)st[lane];
  const uint32_t clen = (sizeof(OutT) == 2 && cls_flag) ? *cls_flag : 0u;
  if (clen && lane < cnt && first + lane < n_settle) {
    const uint32_t e = st[lane];
    const uint8_t* const row = fl + lane * stride;
    const uint32_t eofs = (*reinterpret_cast<const uint16_t*>(row + 10) >> e) & 1u;
    uint32_t nl, full;  // (L + 1)-bit codes on the chain from e; the value that stands for "or more"
    if (clen == 8u) {
      nl = (*reinterpret_cast<const uint32_t*>(row + 12) >> (3u * e)) & 7u;
      full = 7u;
    } else {
      nl = row[5u + (e < 5u ? e : 0u)];
      full = 255u;
    }
    if (e <= clen && nl != full && !eofs) {  // bits from the entry offset to the landing bit = L per code + 1 per long code
      cnt_out[first + lane] = ((uint32_t)kSubBits + row[e] - e - nl) / clen;
      used_out[first + lane] = (uint16_t)e;
      eof_out[first + lane] = 0;  // (a pass that ran on an earlier guess may have seen a fake end mark here)
    }
  }
}

size_t sync_scan_workspace(uint64_t nsub) {
  uint64_t n = nsub, total = 0;
  for (;;) {
    total += n;
    if (n <= 1) break;
    n = (n + 63) / 64;
  }
  return (size_t)(total * (64 + 1) + 256 * 33);  // functions (<= 64 bytes) + entry offsets of every level, each level 256-aligned, + the class flag
}

static uint32_t k6_blocks(uint64_t nsub) {
  const uint64_t groups = (nsub + 63) / 64;
  uint64_t blocks = (groups + kK6Waves - 1) / kK6Waves;
  if (blocks > 256) blocks = 256;  // one workgroup per CU (LDS)
  return blocks ? (uint32_t)blocks : 1u;
}

void launch_sync_scan(const SyncParams& p, uint8_t* ws, uint32_t stride, uint32_t entry, hipStream_t s) {
  if (p.nsub == 0) return;
  // carve: functions of level 0.., then entry offsets of level 1..
  uint64_t cnt[16];
  uint8_t* fn[16];
  uint8_t* st[16];
  int levels = 0;
  uint8_t* q = ws;
  for (uint64_t n = p.nsub;; n = (n + 63) / 64) {
    cnt[levels] = n;
    fn[levels] = q;
    q += (n * stride + 255) & ~(uint64_t)255;
    ++levels;
    if (n <= 1 || levels == 16) break;
  }
  for (int l = 0; l < levels; ++l) {
    st[l] = q;
    q += (cnt[l] + 255) & ~(uint64_t)255;
  }
  uint32_t* const cls_flag = reinterpret_cast<uint32_t*>(q);
  hipLaunchKernelGGL(k_sync_table, dim3(k6_blocks(p.nsub)), dim3(kK6Threads), 0, s, p, stride, fn[0], cls_flag);
  for (int l = 0; l + 1 < levels; ++l)
    hipLaunchKernelGGL(k_fn_reduce, dim3((uint32_t)cnt[l + 1]), dim3(64), 0, s, fn[l], cnt[l], stride, fn[l + 1]);
  // the top level has one element: the whole body, entered at bit `entry` (< stride) of its first subsequence
  if (levels == 1) {
    return;  // a single subsequence: its start is the caller's
  }
  const uint32_t* const no_flag = nullptr;
  hipLaunchKernelGGL(k_fn_apply<uint8_t>, dim3(1), dim3(64), 0, s, fn[levels - 1], cnt[levels - 1], stride, (const uint8_t*)nullptr,
                     entry, st[levels - 1], no_flag, 0ull, (uint32_t*)nullptr, (uint16_t*)nullptr, (uint8_t*)nullptr);
  for (int l = levels - 2; l >= 1; --l)
    hipLaunchKernelGGL(k_fn_apply<uint8_t>, dim3((uint32_t)cnt[l + 1]), dim3(64), 0, s, fn[l], cnt[l], stride, st[l + 1], 0u, st[l], no_flag,
                       0ull, (uint32_t*)nullptr, (uint16_t*)nullptr, (uint8_t*)nullptr);
  // settled by the lowest level (class codes only): whole groups of 64 subsequences, and never the last subsequence (its
  // landing bit, the end of a piece and the end mark are k_sync_pass's)
  uint64_t n_settle = (p.end_bit - p.body_bit0) / (64ull * kSubBits) * 64ull;
  if (n_settle > p.nsub - 1) n_settle = p.nsub - 1;
  hipLaunchKernelGGL(k_fn_apply<uint16_t>, dim3((uint32_t)cnt[1]), dim3(64), 0, s, fn[0], cnt[0], stride, st[1], 0u, p.start,
                     (const uint32_t*)cls_flag, (unsigned long long)n_settle, p.cnt, p.used, p.eof);
}

// first subsequence that holds the end mark (valid once the passes have converged)
__global__ __launch_bounds__(256) void k_sync_eof(SyncParams P) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < P.nsub && P.eof[i]) atomicMin(reinterpret_cast<unsigned long long*>(P.eof_sub), (unsigned long long)i);
}

// symbols per tile of 256 subsequences, nothing counted behind the end mark
__global__ __launch_bounds__(256) void k_sync_tile_sums(SyncParams P) {
  __shared__ unsigned long long ws[4];
  const uint64_t eof_sub = *P.eof_sub;
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  unsigned long long v = (i < P.nsub && i <= eof_sub) ? P.cnt[i] : 0ull;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) P.tile_sum[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}

// absolute bit position of every 64th symbol (the side-car's granularity); a workgroup trip = 1024 subsequences = four of
// the 256-subsequence tiles whose symbol counts k_sync_tile_sums / k_scan prefix-summed
__global__ __launch_bounds__(kK6Threads, 4) void k_sync_index(SyncParams P, uint64_t* __restrict__ seg_abs, uint64_t n_segs, uint64_t n_symbols) {
  GHF_K6_PROLOGUE();
  (void)ngroups;
  const K6Cls CL = k6_cls(k6_mode, P.dt->min_len, max_len, C2, P.body_bit0);
  __shared__ unsigned long long wsum[kK6Waves];
  const uint64_t eof_sub = *P.eof_sub;
  const uint64_t ntrips = (P.nsub + kK6Threads - 1) / kK6Threads;
  auto run = [&](auto mode_tag) {
  constexpr int MODE = decltype(mode_tag)::value;
  for (uint64_t trip = blockIdx.x; trip < ntrips; trip += gridDim.x) {
    const uint64_t g = trip * kK6Waves + wave;  // this wave's group of 64 subsequences
    const uint64_t sub = g * 64 + lane;
    const bool valid = sub < P.nsub && sub <= eof_sub;
    const uint32_t c = valid ? P.cnt[sub] : 0u;
    // exclusive prefix of the symbol counts inside the 256-subsequence tile (4 waves)
    const uint32_t incl = wave_incl_scan_u32(c);
    __syncthreads();  // (the previous trip's readers of wsum are done)
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    unsigned long long first = incl - c;
    if (g * 64 < P.nsub) {
      first += P.tile_sum[g >> 2];  // tile_sum[] holds the exclusive scan by now
      for (int k = wave & ~3; k < wave; ++k) first += wsum[k];
    }
    if (g * 64 >= P.nsub) continue;  // (uniform per wave; the barriers above were passed by everyone)
    wave_sync();
    const uint32_t base = k6_stage(P, g * 64, lin, la0, lane);
    wave_sync();
    const uint32_t limit = k6_limit(body_bits, g);
    const uint64_t abs0 = P.body_bit0 + g * 64 * kSubBits;  // stream bit of the wave's first subsequence
    if (MODE == 2 && CL.L && limit >= 64u * kSubBits) {  // class codes (wave-uniform): the true chain as a walk over the class masks
      auto walk = [&](auto l_tag) {
        constexpr int CLEN = decltype(l_tag)::value;
        uint64_t F[8], G[8];
        k6_classes<CLEN, false>(lin, la0, base + (uint32_t)lane * kSubBits, 0u, F, G);
        k6_mask_t* const Fl = k6_f_slot(L, tid);
#pragma unroll
        for (int r = 0; r < 8; ++r) Fl[r * kK6Threads] = F[r];
        if (!valid || c == 0u) return;
        // symbol numbers m0 (and, L = 4, m0 + 64) of the chain are the first of a segment, symbol number c the first one
        // that is not counted here
        const uint32_t m0 = (uint32_t)((64u - (uint32_t)(first & 63u)) & 63u);
        const uint32_t lo = (uint32_t)lane * kSubBits;
        uint32_t p = P.start[sub], k0 = 0, p_end = 0;
        while (k0 < c) {  // one run of L-bit codes, closed by an (L + 1)-bit code or by the end of the subsequence
          bool found, eof;
          const uint32_t sh = k6_jump<CLEN, false>([&](uint32_t c) { return Fl[c * kK6Threads]; }, [](uint32_t) { return 0ull; }, p, found, eof);
          const uint32_t run = found ? sh + 1u : sh;  // codes in it
#pragma unroll
          for (uint32_t m = m0; m < 64u * (8u / (uint32_t)CLEN); m += 64u) {
            const uint64_t seg = (first + m) >> 6;
            if (m >= k0 && m < k0 + run && m < c && seg < n_segs) seg_abs[seg] = abs0 + lo + p + (uint32_t)CLEN * (m - k0);
          }
          if (c <= k0 + run) p_end = p + (uint32_t)CLEN * (c - k0) + ((found && c == k0 + run) ? 1u : 0u);
          p += (uint32_t)CLEN * sh + (uint32_t)CLEN + 1u;
          k0 += run;
          if (!found) break;  // (the chain has left the subsequence: c <= k0 by the count's definition)
        }
        if (first + c == n_symbols) seg_abs[n_segs] = abs0 + lo + p_end;  // where the last data symbol ends
      };
      if (CL.L == 8) walk(std::integral_constant<int, 8>{});
      else walk(std::integral_constant<int, 4>{});
      continue;
    }
    if (!valid) continue;
    uint32_t pos = (uint32_t)lane * kSubBits + P.start[sub];
    K6Cursor cur;
    cur.open(lin, la0, base + pos);
    uint32_t mark = (uint32_t)((64u - (uint32_t)(first & 63u)) & 63u);  // my symbols in front of the next segment start
    uint64_t seg = (first + mark) >> 6;
    const bool pairs = MODE != 2 && max_len <= 16 && limit >= 64u * kSubBits;  // (wave-uniform; see k_sync_pass)
    for (uint32_t k = 0; k < c && pos < limit;) {
      if (k == mark) {
        if (seg < n_segs) seg_abs[seg] = abs0 + pos;
        ++seg;
        mark += 64u;
      }
      const uint32_t stop = c < mark ? c : mark;  // the next symbol number at which something is written
      if (pairs) {  // (the counts are exact: no end mark among these symbols, none of them behind the stream's end)
        for (; k + 2u <= stop; k += 2u) {
          uint32_t e0, e1;
          k6_peek2<MODE == 2 ? 1 : MODE>(cur, lin, L.t, T1, lut_bits, max_len, e0, e1);
          const uint32_t l = ((e0 >> 8) & 0xFFu) + ((e1 >> 8) & 0xFFu);
          pos += l;
          cur.o += l;
        }
      }
      if (k < stop) {
        pos += (k6_step<MODE>(cur, lin, L.t, T1, lut_bits, max_len, C2) >> 8) & 0xFFu;
        ++k;
      }
    }
    if (c && first + c == n_symbols) seg_abs[n_segs] = abs0 + pos;  // where the last data symbol ends
  }
  };
  if (k6_mode == 2) run(std::integral_constant<int, 2>{});
  else if (k6_mode == 1) run(std::integral_constant<int, 1>{});
  else run(std::integral_constant<int, 0>{});
}

// seg_abs[s] = stream bit of symbol 64 s (s < n_segs), seg_abs[n_segs] = end of the last symbol  ->  the side-car K5 emits:
// absolute start bit per block of 64 segments, end bit of every segment relative to its block
__global__ __launch_bounds__(256) void k_sync_finalize(const uint64_t* __restrict__ seg_abs, uint64_t n_segs,
                                                       uint64_t* __restrict__ chunk_bit, uint32_t* __restrict__ seg_bit) {
  const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= n_segs) return;
  const uint64_t b = s / (kBlockSymbols / kSegSymbols);
  const uint64_t b0 = seg_abs[b * (kBlockSymbols / kSegSymbols)];
  if (s == b * (kBlockSymbols / kSegSymbols)) chunk_bit[b] = b0;
  seg_bit[s] = (uint32_t)(seg_abs[s + 1] - b0);
}

void launch_sync_pass(const SyncParams& p, hipStream_t s) {
  hipLaunchKernelGGL(k_sync_pass, dim3(k6_blocks(p.nsub)), dim3(kK6Threads), 0, s, p);
}
void launch_sync_counts(const SyncParams& p, uint64_t* d_total, hipStream_t s) {
  const uint32_t tiles = (uint32_t)((p.nsub + 255) / 256);
  hipLaunchKernelGGL(k_sync_eof, dim3(tiles), dim3(256), 0, s, p);
  hipLaunchKernelGGL(k_sync_tile_sums, dim3(tiles), dim3(256), 0, s, p);
  launch_scan(p.tile_sum, tiles, d_total, s);
}
void launch_sync_index(const SyncParams& p, uint64_t* d_seg_abs, uint64_t n_symbols, uint64_t* d_chunk_bit, uint32_t* d_seg_bit,
                       hipStream_t s) {
  const uint64_t n_segs = segs_for(n_symbols);
  const uint64_t trips = (p.nsub + kK6Threads - 1) / kK6Threads;
  hipLaunchKernelGGL(k_sync_index, dim3((uint32_t)(trips < 256 ? (trips ? trips : 1) : 256)), dim3(kK6Threads), 0, s, p, d_seg_abs, n_segs, n_symbols);
  if (n_segs) hipLaunchKernelGGL(k_sync_finalize, dim3((uint32_t)((n_segs + 255) / 256)), dim3(256), 0, s, d_seg_abs, n_segs,
                                 d_chunk_bit, d_seg_bit);
}

}  // namespace ghf
