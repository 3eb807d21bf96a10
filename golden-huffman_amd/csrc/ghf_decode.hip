// golden-huffman_amd/csrc/ghf_decode.hip -- the decode-table kernels and K7 (table-driven block-parallel decode),
// gfx950 / wave64.  (K6, the side-car reconstruction for streams that come without one: ghf_sync.hip; the seek table and
// the range head: ghf_seek.hip; what they share: ghf_dec_core.h.)  File:line citations are relative to the reference tree.
#include "ghf_code_rules.h"
#include "ghf_dec_core.h"

namespace ghf {

// ------------------------------------------------------------------------------------------------
// K7: decode.  k_build_decode_tables turns the header tables into left-justified first codes
// (FastCanonicalHuffDecoder, canonical_huff_encoder.cc:433-434) and a 2^lut_bits direct table
// {symbol, length} -- the reference's 8-bit length LUT (canonical_huff_encoder.cc:466-516) widened
// to min(max_len, 12) bits so that no linear extension is needed at any BASELINE config; longer
// codes fall back to the reference's linear search over first_code (cfind, canonical_huff_encoder.h:157-162).
// ------------------------------------------------------------------------------------------------
// DecTables::image from the compact tables (LDS): every table has at least four copies of an entry side by side, so the
// image is written 16 bytes at a time
__device__ __forceinline__ void dec_image_fill(DecTables* __restrict__ dt, const uint16_t* lut, const uint32_t* lut2, int lb, int pb, int tid,
                                               int nthreads) {
  uint4* const img4 = reinterpret_cast<uint4*>(dt->image);
  if (pb) {
    const int r2 = GHF_DEC_COPY_SHIFT(pb);
    // (unrolled sixteen times, as the compiler does now that k_build_decode_tables keeps CodeTab in LDS, that kernel takes 94
    //  registers; the pragma can go if it stops doing so)
#pragma unroll 1
    for (int g = tid; g < (1 << (pb + r2 - 2)); g += nthreads) {
      const uint32_t e = lut2[(4 * g) >> r2];
      img4[g] = make_uint4(e, e, e, e);
    }
    for (int g = tid; g < kDec7SmallSlots / 4; g += nthreads) {
      const uint32_t e = dec7_entry(lut[((4 * g) >> kDecCopyShiftMax) & ((1 << lb) - 1)]);
      img4[kDec7LutSlots / 4 + g] = make_uint4(e, e, e, e);
    }
  } else {
    const int r1 = GHF_DEC_COPY_SHIFT(lb);
    for (int g = tid; g < (1 << (lb + r1 - 2)); g += nthreads) {
      const uint32_t e = dec7_entry(lut[(4 * g) >> r1]);
      img4[g] = make_uint4(e, e, e, e);
    }
  }
}

// (the body of the two kernels below: 256 threads, one workgroup per code)
__device__ __forceinline__ void build_decode_tables(const ghf_code* __restrict__ code, DecTables* __restrict__ dt, int* __restrict__ status) {
  __shared__ CodeTab T;  // fcl / sp / symbol and the one-symbol direct table (ghf_code_rules.h)
  __shared__ unsigned long long kraft;
  __shared__ int bad;
  __shared__ uint32_t s_lut2[1 << kDecPairBitsMax];  // sym0 | sym1 << 8 | (len0 + len1) << 16 ; bit 30 = not two data symbols
  const int tid = threadIdx.x;
  const int max_len = code->max_len, min_len = code->min_len;
  if (!len_bounds_ok(min_len, max_len)) {
    if (tid == 0) latch_status(status, GHF_E_FORMAT);
    return;
  }
  // The tables may come from anywhere (ghf_parse_header checks a header on the host; a caller's own ghf_code is not
  // checked by anyone else): a complete prefix code, or refused (ghf_code_rules.h, section 2).
  if (tid == 0) {
    kraft = 0;
    bad = 0;
  }
  __syncthreads();
  {
    unsigned long long k = 0;
    if (!code_share_ok(code, min_len, max_len, tid, 256, &k)) atomicOr(&bad, 1);
    if (k) atomicAdd(&kraft, k);
  }
  __syncthreads();
  const bool lone_end_mark = max_len == 1 && kraft == (1ull << 31) && code->length[GHF_NSYM - 1] == 1;  // GHF_EMPTY_OK's stream
  if (bad || (kraft != (1ull << 32) && !lone_end_mark)) {
    if (tid == 0) latch_status(status, GHF_E_FORMAT);
    return;
  }
  const int lb = max_len < kDecLutBitsMax ? max_len : kDecLutBitsMax;
  if (tid < 36) {
    tab_load_row(T, tid, min_len, max_len, code->first_code, code->start_pos);
    dt->fc_left[tid] = T.fcl[tid];
    dt->start_pos[tid] = T.sp[tid];
  }
  for (int i = tid; i < GHF_NSYM; i += 256) dt->symbol[i] = T.symbol[i] = tab_symbol(code->symbol[i]);
  // two symbols per lookup when any two codes fit the index (small alphabets: 16-symbol data has max_len 5)
  const int pb = 2 * max_len <= kDecPairBitsMax ? 2 * max_len : 0;
  if (tid == 0) {
    dt->min_len = min_len;
    dt->max_len = max_len;
    dt->lut_bits = lb;
    dt->pair_bits = pb;
    dt->kind = 0;
    dt->root = 0;
    dt->done = 0;
  }
  if (tid < 16) dt->ticket[tid * 32] = 0;
  __syncthreads();
  tab_fill_lut(T, min_len, lb, tid, 256);
  for (uint32_t idx = tid; pb && idx < (1u << pb); idx += 256) {
    const uint32_t v = idx << (32 - pb);
    const uint32_t e0 = tab_search(T, v, min_len, max_len);
    uint32_t ent = (1u << 30) | (1u << 16);  // not a data symbol: flagged, one bit consumed
    if (e0 && (e0 & 0x1FFu) != 256u) {
      const uint32_t l0 = e0 >> 9;
      const uint32_t e1 = tab_search(T, v << l0, min_len, max_len);
      if (e1 && (e1 & 0x1FFu) != 256u) ent = (e0 & 0xFFu) | ((e1 & 0xFFu) << 8) | ((l0 + (e1 >> 9)) << 16);
      else ent = (1u << 30) | (l0 << 16);
    }
    s_lut2[idx] = ent;
  }
  __syncthreads();
  dec_image_fill(dt, T.lut, s_lut2, lb, pb, tid, 256);
}

__global__ __launch_bounds__(256) void k_build_decode_tables(const ghf_code* __restrict__ code, DecTables* __restrict__ dt,
                                                             int* __restrict__ status) {
  build_decode_tables(code, dt, status);
}

// The tables of several codes in ONE launch (ghf_decode_planes_sparse_range from seek tables: up to sixteen stored streams,
// whose tables would otherwise be sixteen launches of one workgroup, one behind the other): workgroup j builds dts[j] from
// codes[j] if bit j of `slots` is set
__global__ __launch_bounds__(256) void k_build_decode_tables_slots(const ghf_code* __restrict__ codes, DecTables* __restrict__ dts, uint32_t slots,
                                                                   int* __restrict__ status) {
  if (!((slots >> blockIdx.x) & 1u)) return;
  build_decode_tables(codes + blockIdx.x, dts + blockIdx.x, status);
}

// .crs: the same direct table, filled by walking the tree DecodeHuffTree::do_build_tree would rebuild
// (include/huff_tree.cc:289-303); what the table cannot resolve is walked bit by bit like decode_byte does (:255-271).
__global__ __launch_bounds__(256) void k_crs_decode_tables(const ghf_tree* __restrict__ tree, DecTables* __restrict__ dt,
                                                           int* __restrict__ status) {
  __shared__ uint16_t tl[256], tr[256];
  __shared__ uint32_t s_min;
  __shared__ uint16_t s_lut[1 << kDecLutBitsMax];
  const int tid = threadIdx.x;
  const int max_len = (int)tree->max_len;
  const uint32_t root = tree->root, nl = tree->n_leaves;
  if (max_len < 1 || max_len > 64 || nl < 2 || nl > 256 || root < 256 || root >= 256 + nl - 1) {
    if (tid == 0) latch_status(status, GHF_E_FORMAT);
    return;
  }
  tl[tid] = tree->left[tid];
  tr[tid] = tree->right[tid];
  if (tid == 0) s_min = 64;
  __syncthreads();
  const int lb = max_len < kDecLutBitsMax ? max_len : kDecLutBitsMax;
  dt->tl[tid] = tl[tid];
  dt->tr[tid] = tr[tid];
  if (tid < 36) {
    dt->fc_left[tid] = 0xFFFFFFFFu;
    dt->start_pos[tid] = 0;
  }
  for (int i = tid; i < GHF_NSYM; i += 256) dt->symbol[i] = 256;
  if (tid < 16) dt->ticket[tid * 32] = 0;
  uint32_t mn = 64;
  for (uint32_t idx = tid; idx < (1u << lb); idx += 256) {
    uint32_t node = root;
    uint16_t ent = 0;
    for (int l = 1; l <= lb; ++l) {
      const uint32_t p = node - 256u;
      if (p >= nl - 1) break;  // a child id that is neither a leaf nor one of the nl - 1 parents: malformed, entry stays 0
      node = ((idx >> (lb - l)) & 1u) ? tr[p] : tl[p];
      if (node < 256u) {
        ent = (uint16_t)(node | ((uint32_t)l << 9));
        mn = (uint32_t)l < mn ? (uint32_t)l : mn;
        break;
      }
    }
    s_lut[idx] = ent;
  }
  atomicMin(&s_min, mn);
  __syncthreads();
  if (tid == 0) {
    dt->min_len = (int32_t)(s_min <= (uint32_t)lb ? s_min : (uint32_t)lb);
    dt->max_len = max_len;
    dt->lut_bits = lb;
    dt->pair_bits = 0;
    dt->kind = 1;
    dt->root = root;
    dt->done = 0;
  }
  dec_image_fill(dt, s_lut, nullptr, lb, 0, tid, 256);
}

void launch_crs_decode_tables(const ghf_tree* d_tree, DecTables* d_dt, int* d_status, hipStream_t s) {
  hipLaunchKernelGGL(k_crs_decode_tables, dim3(1), dim3(256), 0, s, d_tree, d_dt, d_status);
}

void launch_build_decode_tables(const ghf_code* d_code, DecTables* d_dt, int* d_status, hipStream_t s) {
  hipLaunchKernelGGL(k_build_decode_tables, dim3(1), dim3(256), 0, s, d_code, d_dt, d_status);
}
void launch_build_decode_tables_slots(const ghf_code* d_codes, DecTables* d_dts, uint32_t count, uint32_t slots, int* d_status, hipStream_t s) {
  if (count == 0 || slots == 0) return;
  hipLaunchKernelGGL(k_build_decode_tables_slots, dim3(count), dim3(256), 0, s, d_codes, d_dts, slots, d_status);
}

template <bool STAGED>
struct DecIn {
  const uint8_t* lin;   // staged: L.in
  uint32_t la0;         // staged: logical byte address of the wave's tile
  const uint8_t* src;   // unstaged: raw bytes of the span
  uint64_t span;
  __device__ __forceinline__ uint32_t fetch(uint32_t widx) const {
    if (STAGED) return in_word(lin, la0 + 4u * widx);
    const uint64_t b = (uint64_t)widx * 4;
    uint32_t r = 0;
    for (int k = 0; k < 4; ++k) r = (r << 8) | (b + k < span ? (uint32_t)src[b + k] : 0u);
    return r;
  }
};

// The hot loops' window (ghf_dec_core.h) over the wave's tile.  K symbols are decoded between two refill checks --
// K * max_len <= 32 keeps o + max_len <= 64 at every lookup.  Macros over the loops' own variables: with a cursor struct
// in their place (K6Cursor's form) the listing of k_decode changes, and that kernel carries the benchmark.
#define GHF_REFILL()           \
  if (o >= 32u) {              \
    win_shift(W, nextw, o);    \
    nextw = in_word(lin, la);  \
    la += 4u;                  \
  }
#define GHF_WINDOW_OPEN()                                              \
  uint32_t la = la0 + ((pos >> 5) << 2);                               \
  uint32_t o = pos & 31u;                                              \
  uint64_t W = win_open(in_word(lin, la), in_word(lin, la + 4u));      \
  uint32_t nextw = in_word(lin, la + 8u);                              \
  la += 12u
#define GHF_WINDOW_USED() ((la - la0 - 12u) * 8u + o - pos)  // (la - la_first - 12) * 8 + o - o0, la_first and o0 being pos's two halves

// HOT: the 64 symbols of a full, staged segment; the 64 bytes stay in registers.  LONG: codes beyond the direct table exist
// (max_len > 12: Zipf 1.1 over 256 values has 13..14-bit codes for its rarest ones and the end mark at 256 MiB) and take the
// reference's linear extension on a miss.  Returns the OR of all entries (kEntEnd / kEntNone set: not 64 data symbols ->
// corrupt).  Every variant ends in the same four stores (the callers' copy-out), so that the compiler can count the kernel's
// memory operations whichever variant runs.
//
// A LOOP, not 64 unrolled lookups: the straight-line form of round 3 (and of this round's first build) made a pass 8..9 KB of
// code and kept 39 registers more alive.  (Code size itself is NOT what that costs: loop bodies up to 16 KB issue at the full
// rate, scratch/ifetch2.hip, profiles/r04/experiments/ifetch2.txt -- the "cliff at 4 KB" an earlier micro-benchmark showed was a
// macro that repeated twice as often as its name said.)  The body is one period of the refill pattern -- lcm(4, K) symbols,
// at most 12 = about 0.8 KB -- and the decoded dwords go to out[] through the uniform loop counter (s_set_gpr_idx: no
// scratch); with 89 registers a K7 workgroup shares its CU with the one-wave code build of a later step.
typedef uint32_t DecOut __attribute__((ext_vector_type(16)));  // a lane's 64 decoded bytes: a register TUPLE, so that out[t] with a
                                                                // uniform t is an indexed register move and never memory
template <int K, bool LONG>
__device__ __forceinline__ uint32_t dec_hot(const DecLds& L, const uint8_t* lin, uint32_t la0, const DecLut& T, int lut_bits, int max_len, uint32_t pos,
                                            DecOut& out, uint32_t& used) {
  GHF_WINDOW_OPEN();
  uint32_t acc = 0;
  constexpr int PER = (K == 3) ? 3 : 1;  // dwords per trip: the refill checks of a trip sit at the same symbols in every trip
  auto dword = [&](int sym0) -> uint32_t {  // symbols sym0 .. sym0 + 3 of the trip -> one output dword
    uint32_t e[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if ((sym0 + j) % K == 0) GHF_REFILL();
      const uint32_t v = win_peek(W, o);
      uint32_t ent = dec_lookup(T, v);
      if (LONG && __builtin_expect((ent & kEntNone) != 0, 0)) ent = dec_long_entry(L, v, lut_bits, max_len);
      o += (ent >> 8) & 0xFFu;
      e[j] = ent;
    }
    acc |= e[0] | e[1] | e[2] | e[3];
    // byte 0 of four entries -> one dword (v_perm_b32): {a.b0, b.b0} then {lo16, hi16}
    const uint32_t lo = __builtin_amdgcn_perm(e[1], e[0], 0x0C0C0400u);
    const uint32_t hi = __builtin_amdgcn_perm(e[3], e[2], 0x0C0C0400u);
    return __builtin_amdgcn_perm(hi, lo, 0x05040100u);
  };
#pragma unroll 1
  for (int t = 0; t < 16 / PER; ++t) {
#pragma unroll
    for (int i = 0; i < PER; ++i) out[t * PER + i] = dword(4 * i);
  }
#pragma unroll
  for (int d = 16 / PER * PER; d < 16; ++d) out[d] = dword(4 * d);  // (K = 3: the sixteenth dword; 60 is a multiple of 3)
  used = GHF_WINDOW_USED();
  return acc;
}

// HOT, small alphabet (2 * max_len <= 10): any two codes fit lut2's index, so one lookup yields two symbols and the serial
// shift -> lookup -> add chain is half as long.  Three lookups (<= 30 bits) per refill check: a trip is six lookups, three dwords.
// entry = sym0 | sym1 << 8 | (len0 + len1) << 16 | bit 30: not two data symbols
__device__ __forceinline__ uint32_t dec_hot_pair(const uint8_t* lin, uint32_t la0, const DecLut& T2, uint32_t pos, DecOut& out, uint32_t& used) {
  GHF_WINDOW_OPEN();
  uint32_t acc = 0;
  auto dword = [&](int look0) -> uint32_t {  // lookups look0, look0 + 1 of the trip -> four symbols
    uint32_t e[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if ((look0 + j) % 3 == 0) GHF_REFILL();
      const uint32_t ent = dec_lookup(T2, win_peek(W, o));
      o += (ent >> 16) & 0xFFu;
      e[j] = ent;
    }
    acc |= e[0] | e[1];
    return __builtin_amdgcn_perm(e[1], e[0], 0x05040100u);  // {a.sym0, a.sym1, b.sym0, b.sym1}
  };
#pragma unroll 1
  for (int t = 0; t < 5; ++t) {
#pragma unroll
    for (int i = 0; i < 3; ++i) out[t * 3 + i] = dword(2 * i);
  }
  out[15] = dword(30);
  used = GHF_WINDOW_USED();
  return acc;
}

#undef GHF_REFILL
#undef GHF_WINDOW_OPEN
#undef GHF_WINDOW_USED

// COLD: whatever the hot passes do not take -- the stream's last group (ragged, followed by the end mark), spans that do
// not fit the LDS tile (read from memory), unaligned output.  One symbol at a time, one byte per store.
template <bool STAGED>
__device__ __forceinline__ uint32_t dec_cold(const DecLds& L, const DecIn<STAGED>& I, const DecLut& T, int lut_bits, int max_len,
                                             uint64_t pos, uint32_t cnt, bool valid, uint8_t* optr, int has_next,
                                             uint64_t expect_bits) {
  if (!valid) return 0u;
  uint32_t widx = (uint32_t)(pos >> 5);
  uint32_t o = (uint32_t)(pos & 31u);
  const uint32_t o0 = o, widx0 = widx;
  // (win_open written out: as its arguments both words are fetched before they are combined -- one instruction of k_decode moves)
  uint64_t W = ((uint64_t)I.fetch(widx) << 32) | I.fetch(widx + 1);
  uint32_t nextw = I.fetch(widx + 2);
  widx += 3;
  uint32_t acc = 0;
  auto one = [&]() -> uint32_t {
    while (o >= 32u) {  // (a code of up to 64 bits moves the cursor by up to two words)
      win_shift(W, nextw, o);
      nextw = I.fetch(widx++);
    }
    const uint32_t v = win_peek(W, o);
    uint32_t ent = dec_lookup(T, v);
    if (ent & kEntNone) ent = dec_long_entry_at(L, W, nextw, o, lut_bits, max_len);
    o += (ent >> 8) & 0xFFu;
    return ent;
  };
  for (uint32_t i = 0; i < cnt; ++i) {
    const uint32_t ent = one();
    acc |= ent;
    optr[i] = (uint8_t)ent;
  }
  // the index says where the next segment starts: an end-to-end check of every segment
  if (has_next == 1) {
    const uint64_t used = (uint64_t)(widx - widx0 - 3) * 32 + o - o0;
    if (used != expect_bits) acc |= kEntNone;
  } else if (has_next == 0) {
    if (!(one() & kEntEnd)) acc |= kEntNone;  // canonical_huff_encoder.cc:404: the end mark must follow
  }
  return acc;
}

// K7.  Persistent waves; each pass a wave takes one side-car block = 64 consecutive segments (4096 symbols):
//   1. the compressed span of the block (known from the side-car) is copied into LDS with coalesced 16-byte loads,
//      byte-swapped to big-endian words;
//   2. every lane decodes its 64 symbols from a 64-bit window: one LDS table lookup per symbol, the 64 bytes stay in
//      registers;
//   3. the wave's 4 KiB of output go through the (now dead) input tile and leave as four coalesced 1 KiB stores.
// The loop is software-pipelined over groups so that no HBM latency is exposed and nothing but the copy into LDS stands
// between the arrival of a span and the request for the next one: while group i is decoded, the span of group i+1 is in
// flight into registers, the descriptor of group i+1 (where to load, where every lane starts) was computed a pass earlier,
// the side-car words of group i+2 are in flight and the ticket for group i+3 is in flight.
//
// Round 3's form of this loop computed the next group's descriptor between the copy into LDS and the loads, held six
// instantiations of the whole loop nest (one per decoder variant, each with its own cold path) and was spilled by the
// register allocator INSIDE the hot loop of the variants uniform bytes take: the fifth vector of the prefetch went to
// scratch right behind its load, i.e. behind an s_waitcnt vmcnt(0) -- every pass waited for the whole prefetch before it
// decoded a symbol, the loads never overlapped the decode (profiles/r04/k7_spill_r03.txt has the listing).  Now: ONE loop,
// the variant is a switch around the 64 lookups only, one cold path, and a CPU-side guard keeps the kernel scratch-free
// (tests/test_cabi_cpu.py).
struct DecMeta {   // side-car words of one group, as loaded: issued a whole pass before they are combined
  uint64_t blk;    // block start (same word in every lane)
  uint32_t end;    // where MY segment ends, relative to blk
};

constexpr uint32_t kDecBadSeg = 0xFFFFFFFFu;
struct DecGroup {       // one group, ready to be fetched and decoded
  const uint8_t* base;  // uniform: what the span loads are relative to (the span's first byte, 16-aligned)
  uint32_t lim;         // uniform: the vector at byte offset o of the span is loaded iff o + 16 <= lim
  uint64_t byte0;       // uniform: first staged byte (16-aligned)
  uint32_t span;        // uniform: staged bytes
  uint32_t pos;         // bit of the staged span at which my segment starts
  uint32_t expect;      // bits of my segment; kDecBadSeg: my side-car words are implausible (no decode consumes that many bits)
  bool hot;             // uniform: complete, staged, plausible, not the stream's last group
};

struct DecConst {  // wave-uniform facts of one launch
  uint64_t n_segs, stream_bytes, stream_end_bit, full_bytes;
  uint32_t ngroups;
  int max_len;
  bool hot_ok;  // the output is 16-byte aligned and no code is longer than 32 bits
};

__device__ __forceinline__ void dec_issue_meta(const DecParams& P, const DecConst& C, uint32_t group, int lane, DecMeta& M) {
  const uint64_t last = C.n_segs - 1;
  const uint64_t seg = (uint64_t)group * 64 + lane;
  M.blk = P.chunk_bit[group];
  M.end = P.seg_bit[seg < last ? seg : last];  // clamped: unconditional loads
}

__device__ __forceinline__ void dec_group(const DecParams& P, const DecConst& C, uint32_t group, int lane, const DecMeta& M, DecGroup& G) {
  const uint64_t seg0 = (uint64_t)group * 64;
  const bool valid = seg0 + lane < C.n_segs;
  const uint64_t B0 = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(M.blk >> 32)) << 32) |
                      (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)M.blk);
  // my segment starts where my left neighbour's ends (v_mov_dpp wave_shr:1; lane 0 starts with the block)
  const uint32_t start = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)M.end, 0x138, 0xF, 0xF, true);
  uint64_t B1 = B0 + (uint32_t)__builtin_amdgcn_readlane((int)M.end, 63);
  const bool last_group = seg0 + 64 >= C.n_segs;
  if (last_group) {
    // last group: bound it by its last segment's worst case (+ end mark) rather than by a side-car word.  Segment starts
    // grow with the lane (a side-car that says otherwise is caught by `bad`), so the last valid lane's start is the largest
    const uint32_t lastv = (uint32_t)(C.n_segs - 1 - seg0) & 63u;
    B1 = B0 + (uint32_t)__builtin_amdgcn_readlane((int)start, (int)lastv) + 65u * (uint32_t)C.max_len;
  }
  if (B1 > C.stream_end_bit) B1 = C.stream_end_bit;
  G.byte0 = (B0 >> 3) & ~15ull;
  uint64_t byte1 = ((B1 + 7) >> 3) + 12;  // window look-ahead
  if (byte1 > C.stream_bytes) byte1 = C.stream_bytes;
  if (G.byte0 > byte1) G.byte0 = byte1 & ~15ull;  // corrupt side-car: caught by `bad`
  const uint64_t span = byte1 - G.byte0;
  G.span = span > 0x7FFFFFFFull ? 0x7FFFFFFFu : (uint32_t)span;
  G.pos = (uint32_t)(B0 & 127u) + start;
  const bool bad = valid && (M.end < start || B0 + M.end > C.stream_end_bit || B0 >= C.stream_end_bit);
  G.expect = bad ? kDecBadSeg : M.end - start;
  // vector k of a lane = bytes byte0 + k * 1024 + lane * 16 .. of the stream; it is loaded when it begins inside the span
  // and ends inside the stream's whole 16-byte vectors:  o + 16 <= lim  <=>  o < span && byte0 + o + 16 <= full_bytes
  uint32_t lim = 0;
  if (G.byte0 <= C.full_bytes) {
    const uint64_t room = C.full_bytes - G.byte0;
    const uint64_t a = (uint64_t)G.span + 15u;
    lim = (uint32_t)(a < room ? a : (room > 0x7FFFFFFFull ? 0x7FFFFFFFull : room));
  }
  G.lim = lim;
  G.base = P.stream + (lim ? G.byte0 : 0ull);
  G.hot = C.hot_ok && !last_group && G.span <= (uint32_t)kDec7InBytes && G.byte0 + G.span <= C.full_bytes && __ballot(bad) == 0;
}

// latch_status whose operands are materialised where it stands (the optimiser otherwise builds the compare-and-swap's
// register pair in front of the loop and keeps it alive -- in scratch -- across all of it)
__device__ __forceinline__ void latch_status_here(int* st, int code) {
  int want = 0;
  asm volatile("" : "+v"(code), "+v"(want));
  atomicCAS(st, want, code);
}

constexpr int kDecVec = (kDec7InBytes + 1023) / 1024;  // 16-byte vectors per lane that cover a staged span

__global__ __launch_bounds__(kDec7Threads) void k_decode(DecParams P) {
  __shared__ DecLds7 L;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform -> scalar loop control
  DecConst C;
  C.n_segs = P.n_segs;
  C.stream_bytes = P.stream_bytes;
  C.stream_end_bit = P.stream_bytes * 8;
  C.full_bytes = P.stream_bytes & ~15ull;  // whole 16-byte vectors of the stream
  // (group numbers are 32-bit -- launch_decode refuses more -- so that the loop control is scalar compares of single
  //  registers: gfx9 has no scalar 64-bit ordering compare)
  C.ngroups = (uint32_t)((P.n_segs + 63) >> 6);
  const uint32_t ngroups = C.ngroups, glast = ngroups - 1;
  auto clampg = [&](uint32_t g) { return g < ngroups ? g : glast; };  // past the end: redundant, harmless loads
  // Groups.  A wave owns ONE group by its number (wid); every other one comes from a ticket counter, so that a workgroup that
  // starts late (a 16-wave workgroup needs a whole CU: one wave of another kernel on it -- K2 of a later step in the
  // pipelined bench -- and it waits for that kernel or for another K7 workgroup to end) owns 16 groups, not more: round 3 gave
  // every wave three groups and the first form of this loop four, and in the pipelined bench that workgroup's 64 groups ran
  // alone behind everybody else's last one (decode 0.135 ms alone, 0.159 in the pipeline).  16 classes of workgroups, one
  // counter each on its own 128-byte line (one word saturates at ~88 tickets per microsecond); class c owns the ticketed
  // groups == c (mod 16).  The first ticket is worth two groups (the depth of the pipeline) and is drawn before the
  // tables are copied in, which hides its round trip.
  const uint32_t nwaves = gridDim.x * kDec7Waves;
  const uint32_t wid = blockIdx.x * kDec7Waves + (uint32_t)wave;
  // A class's workgroups are spread over all eight XCDs (consecutive workgroups go to consecutive XCDs): a class is a
  // fixed share of the groups, and an XCD that runs slower than the others would otherwise finish its classes last.
  const uint32_t ncls = gridDim.x < 16u ? 1u : (gridDim.x < 128u ? gridDim.x >> 3 : 16u);  // every class needs at least one workgroup
  const uint32_t cls = (blockIdx.x >> 3) % ncls;
  uint32_t* const my_ticket = &P.dt->ticket[cls * 32];
  auto claim_issue = [&](unsigned int count) -> unsigned int {  // the atomic's return value stays in a VGPR until claim_group() needs it, a pass later
    unsigned int t = 0;
    if (lane == 0) t = atomicAdd(my_ticket, count);
    return t;
  };
  auto claim_group = [&](unsigned int t, uint32_t k) -> uint32_t {  // group of ticket t + k (saturating: past the end stays past the end)
    const uint64_t g = (uint64_t)nwaves + ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)t) + k) * ncls + cls;
    return g < 0xFFFFFFFFull ? (uint32_t)g : 0xFFFFFFFFu;
  };
  uint32_t g0 = wid, g1, g2;
  const unsigned int tk0 = claim_issue(2);

  // The first two groups' side-car words are requested BEFORE the tables are pulled in: one of the dependent memory round
  // trips in front of the first decode hides behind the table copy.
  DecMeta M0, M;
  dec_issue_meta(P, C, clampg(g0), lane, M0);
  if (tid == 0) L.t.status0 = *P.status;  // one read per workgroup: whether the launch does anything must be uniform
  const int lut_bits = P.dt->lut_bits, max_len = P.dt->max_len;
  const int pair_bits = P.dt->pair_bits;
  dec_lds_load(L.t, P.dt, tid, kDec7Threads);
  if (blockIdx.x == 0 && tid == 0 && P.out_bytes) *P.out_bytes = P.n_symbols;
  __syncthreads();
  C.max_len = max_len;
  C.hot_ok = (((uintptr_t)P.out) & 15u) == 0 && max_len <= 32;  // codes beyond 32 bits (a very deep .crs tree): one symbol at a time

  if (L.t.status0 == 0 && g0 < ngroups) {
    // a lane's replicas of the tables: T1 = one symbol per lookup, T2 = two (small alphabets only).  The uniform parts live in
    // SGPRs, the lane's part is recomputed in every pass (two VALU instructions instead of two registers).  (The uniform parts
    // are spelled out here as dec_lut1 / dec_lut2 compute them: calling those from the lambdas changes this kernel's listing.)
    const int r1 = pair_bits ? kDecCopyShiftMax : GHF_DEC_COPY_SHIFT(lut_bits);
    const int r2 = GHF_DEC_COPY_SHIFT(pair_bits);
    const uint32_t* const t1 = L.t.lut + (pair_bits ? kDec7LutSlots : 0);
    auto lut1 = [&](int ln) { return dec_replica(t1, lut_bits, r1, ln); };
    auto lut2 = [&](int ln) { return dec_replica(L.t.lut, pair_bits, r2, ln); };
    // decoder variant (wave-uniform): 0 pair table; 1..3 K = 4 / 3 / 2 symbols per refill check; 4, 5 codes beyond the table
    // K = 32 / max_len symbols per refill check (o <= 31 behind a check, o + K * max_len <= 63 before the next: a single
    // refill brings it back below 32.  With 33 -- max_len 11, K = 3 -- o could reach 64, stay at 32 behind the refill, and
    // the third lookup of the next round would read past the window: six 11-bit codes in a row at the right phase, found by
    // scratch/host_soak.py)
    const int var = pair_bits ? 0 : max_len <= 8 ? 1 : max_len <= 10 ? 2 : max_len <= kDecLutBitsMax ? 3 : max_len <= 16 ? 4 : 5;
    const uint8_t* const lin = L.in;
    const uint32_t la0 = (uint32_t)wave * kDec7TileLog;             // this wave's tile in the logical (unpadded) byte space
    uint32_t* const tile = reinterpret_cast<uint32_t*>(L.in + (uint32_t)wave * kDec7TilePhys);  // ... and as plain memory (copy-out)
    uint32_t bad_acc = 0;

    auto issue = [&](const DecGroup& G, uint4 (&R)[kDecVec], int ln) {
#pragma unroll
      for (int k = 0; k < kDecVec; ++k) {  // lanes behind the span re-read the span's first bytes (an L2 hit)
        const uint32_t o = (uint32_t)k * 1024u + (uint32_t)ln * 16u;
        R[k] = load_stream(G.base + (o + 16u <= G.lim ? o : 0u));  // read once: not worth a line of the Infinity Cache
      }
    };

    DecGroup cur, nxt;
    uint4 R[kDecVec];
    dec_group(P, C, clampg(g0), lane, M0, cur);
    issue(cur, R, lane);
    g1 = claim_group(tk0, 0);
    g2 = claim_group(tk0, 1);
    dec_issue_meta(P, C, clampg(g1), lane, M);
    unsigned int tk = claim_issue(1);  // for the group after g2
    dec_group(P, C, clampg(g1), lane, M, nxt);  // (the one dependent side-car round trip of a wave's life; the first span is in flight meanwhile)
    dec_issue_meta(P, C, clampg(g2), lane, M);

    // One pass over a group.  HOT = the group is complete, staged, plausible and not the stream's last: the body then has
    // no data-dependent branch around its memory operations, so the compiler can count them -- the wait for the
    // prefetched span becomes "all but the youngest seven" (this group's output stores, the next side-car words, the
    // ticket) instead of vmcnt(0), and the wave never sleeps until its own stores are acknowledged by L2.
    auto pass = [&](auto hot_tag) {
      constexpr bool HOT = decltype(hot_tag)::value;
      // the lane number, recomputed (v_mbcnt) and opaque to the optimiser: everything derived from it below (a dozen LDS and
      // global addresses) costs a few VALU instructions per pass instead of registers that live across the whole loop
      int ln = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
      asm volatile("" : "+v"(ln));
      // ---- 1. this group's span: registers -> LDS (big-endian words).  HOT: whatever a lane loaded behind the span is
      // harmless (only a corrupt stream reads it, and that is caught by the segment-end check); else it reads as zero
      wave_sync();
#pragma unroll
      for (int k = 0; k < kDecVec; ++k) {
        const uint32_t o = (uint32_t)k * 1024u + (uint32_t)ln * 16u;
        uint4 v = R[k];
        v = make_uint4(bswap32(v.x), bswap32(v.y), bswap32(v.z), bswap32(v.w));
        if (!HOT && !(o + 16u <= cur.lim)) v = make_uint4(0, 0, 0, 0);
        if ((k + 1) * 1024 <= kDec7InBytes || o < (uint32_t)kDec7InBytes)
          *reinterpret_cast<uint4*>(L.in + in_phys(la0 + o)) = v;
      }
      if (ln < 4) *reinterpret_cast<uint32_t*>(L.in + in_phys(la0 + kDec7InBytes + 4u * ln)) = 0;
      if (!HOT && cur.byte0 + cur.span > C.full_bytes && C.full_bytes >= cur.byte0 && ln == 0) {
        // the stream's last, incomplete 16 bytes: byte loads, never past the end of the buffer
        uint32_t q[4] = {0, 0, 0, 0};
        for (uint64_t j = 0; C.full_bytes + j < C.stream_bytes; ++j) q[j >> 2] |= (uint32_t)P.stream[C.full_bytes + j] << (24 - 8 * (j & 3));
        const uint64_t w = (C.full_bytes - cur.byte0) >> 2;
        if (w + 3 < (uint64_t)kDec7InWords + 4) {
          for (int j = 0; j < 4; ++j) *reinterpret_cast<uint32_t*>(L.in + in_phys(la0 + 4u * (uint32_t)(w + j))) = q[j];
        }
      }
      wave_sync();
      // ---- 2. the next group's span is requested at once: its descriptor was computed a pass ago
      issue(nxt, R, ln);
      // ---- 3. decode
      const uint64_t seg0 = (uint64_t)g0 * 64;
      const uint64_t seg = seg0 + ln;
      const uint64_t sym0 = seg * kSegSymbols;
      if (HOT) {
        uint32_t used, acc;
        DecOut out;
        if (var == 0) acc = dec_hot_pair(lin, la0, lut2(ln), cur.pos, out, used) >> 14;  // bit 30 -> bit 16
        else if (var == 1) acc = dec_hot<4, false>(L.t, lin, la0, lut1(ln), lut_bits, max_len, cur.pos, out, used);
        else if (var == 2) acc = dec_hot<3, false>(L.t, lin, la0, lut1(ln), lut_bits, max_len, cur.pos, out, used);
        else if (var == 3) acc = dec_hot<2, false>(L.t, lin, la0, lut1(ln), lut_bits, max_len, cur.pos, out, used);
        else if (var == 4) acc = dec_hot<2, true>(L.t, lin, la0, lut1(ln), lut_bits, max_len, cur.pos, out, used);
        else acc = dec_hot<1, true>(L.t, lin, la0, lut1(ln), lut_bits, max_len, cur.pos, out, used);
        // copy-out through the input tile (dead now): lane-major 64-byte rows, pieces XOR-swizzled so that the 16
        // lanes of a write phase hit 16 different bank groups; then four fully coalesced 1 KiB stores per wave,
        // straight-line, so that the compiler can count them
        wave_sync();
        const uint32_t osw = ((uint32_t)ln >> 2) & 3u;
#pragma unroll
        for (int q = 0; q < 4; ++q)
          *reinterpret_cast<uint4*>(tile + ln * 16 + (((uint32_t)q ^ osw) << 2)) = make_uint4(out[4 * q], out[4 * q + 1], out[4 * q + 2], out[4 * q + 3]);
        wave_sync();
        uint8_t* og = P.out + seg0 * kSegSymbols + (uint32_t)ln * 16;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const uint32_t sl = (uint32_t)r * 16 + ((uint32_t)ln >> 2);  // the lane whose row holds my piece
          const uint32_t piece = ((uint32_t)ln & 3u) ^ ((sl >> 2) & 3u);
          store_stream(og + r * 1024, *reinterpret_cast<const uint4*>(tile + sl * 16 + piece * 4));
        }
        if (used != cur.expect) acc |= kEntNone;
        bad_acc |= acc;
      } else {
        const bool valid = seg < C.n_segs;
        if (__ballot(cur.expect == kDecBadSeg)) {
          if (cur.expect == kDecBadSeg) latch_status_here(P.status, GHF_E_CORRUPT);
        } else {
          const bool staged = cur.span <= (uint32_t)kDec7InBytes;
          uint32_t cnt = 0;
          if (valid) cnt = (P.n_symbols - sym0 >= (uint64_t)kSegSymbols) ? (uint32_t)kSegSymbols : (uint32_t)(P.n_symbols - sym0);
          // 1: the side-car says where the next segment starts; 0: the end mark must follow; 2: nothing to check
          const int has_next = seg + 1 < C.n_segs ? 1 : (P.no_end_mark ? 2 : 0);
          const uint8_t* src = P.stream + cur.byte0;
          if (staged) {
            DecIn<true> I{lin, la0, src, cur.span};
            bad_acc |= dec_cold<true>(L.t, I, lut1(ln), lut_bits, max_len, cur.pos, cnt, valid, P.out + sym0, has_next, cur.expect);
          } else {
            DecIn<false> I{lin, la0, src, cur.span};
            bad_acc |= dec_cold<false>(L.t, I, lut1(ln), lut_bits, max_len, cur.pos, cnt, valid, P.out + sym0, has_next, cur.expect);
          }
        }
      }
      // ---- 4. behind the decode, where nothing waits for it: the descriptor of the group after the next (its side-car
      // words were requested a pass ago), the side-car words of the one after that, the number of the one after that
      cur = nxt;
      dec_group(P, C, clampg(g2), ln, M, nxt);
      g0 = g1;
      g1 = g2;
      g2 = claim_group(tk, 0);  // (drawn a pass ago: a wave holds two groups beyond the one it decodes -- what it still has to do
                                //  when the counters run dry is the launch's tail)
      dec_issue_meta(P, C, clampg(g2), ln, M);
      tk = claim_issue(1);
    };
    while (g0 < ngroups) {
      if (cur.hot) {
        // drain once on entry: the hot loop's waits are then computed from its own back edge alone (exact counts)
        // instead of being merged with whatever the cold paths left outstanding
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
        do pass(std::true_type{});
        while (g0 < ngroups && cur.hot);
      }
      if (g0 < ngroups) pass(std::false_type{});
    }
    if (bad_acc & (kEntEnd | kEntNone)) latch_status_here(P.status, GHF_E_CORRUPT);  // 64 data symbols per full segment, always
  }
  // the last workgroup to finish hands the ticket counters back as it found them
  __syncthreads();
  if (tid == 0) {
    const unsigned int arrived = atomicAdd(&P.dt->done, 1u);
    if (arrived == gridDim.x - 1) {
      for (int k = 0; k < 16; ++k) __hip_atomic_store(&P.dt->ticket[k * 32], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&P.dt->done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

void launch_decode(const DecParams& p, hipStream_t s) {
  const uint64_t groups = (p.n_segs + 63) / 64;
  uint64_t blocks = (groups + kDec7Waves - 1) / kDec7Waves;
  if (blocks == 0) return;
  if (groups >= kDecMaxGroups) return;  // (k_decode numbers its groups in 32 bits; the callers refuse such an index first)
  if (blocks > 256) blocks = 256;  // persistent: one workgroup of 16 waves per CU (its LDS tiles + table take 153 KiB)
  hipLaunchKernelGGL(k_decode, dim3((uint32_t)blocks), dim3(kDec7Threads), 0, s, p);
}

}  // namespace ghf
