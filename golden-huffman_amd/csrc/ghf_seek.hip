// golden-huffman_amd/csrc/ghf_seek.hip -- the seek table (k_seek_pack, k_seek_expand) and the range head (k_decode_head),
// gfx950 / wave64.
#include "ghf_dec_core.h"

namespace ghf {

// ------------------------------------------------------------------------------------------------
// The seek table (no reference counterpart: the .crs2 wire format has no sync points; DESIGN.md "Seekable .crs2"):
// the side-car in a form small enough to keep beside the file.  Per block of 4096 symbols the absolute start bit and
// the bit lengths of its eight runs of 512 symbols; k_seek_expand turns that back into the full side-car by decoding
// code LENGTHS only, one lane per run.  A table comes from disk: nothing in it is trusted.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_seek_pack(SeekPackParams P) {
  const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  uint64_t* const t64 = reinterpret_cast<uint64_t*>(P.table);
  if (g == 0) {
    t64[0] = kSeekMagic;
    t64[1] = (uint64_t)kSeekVersion | ((uint64_t)P.flags << 32);
    t64[2] = P.n_symbols;
    t64[3] = (uint64_t)kBlockSymbols | ((uint64_t)kRunSymbols << 32);
    t64[4] = P.n_blocks;
    t64[5] = 0;
    t64[6] = 0;
    t64[7] = 0;
  }
  if (g >= P.n_blocks) return;
  const uint64_t seg0 = g * (kBlockSymbols / kSegSymbols);
  uint32_t prev = 0, bad = 0;
  uint64_t w[2] = {0, 0};
#pragma unroll
  for (int k = 0; k < kRunsPerBlock; ++k) {
    const uint64_t first = seg0 + (uint64_t)k * kRunSegs;
    uint32_t r = 0;
    if (first < P.n_segs) {
      const uint64_t last = first + kRunSegs - 1;
      const uint32_t e = P.seg_bit[last < P.n_segs ? last : P.n_segs - 1];
      r = e - prev;
      prev = e;
    }
    bad |= r > 0xFFFFu ? 1u : 0u;
    w[k >> 2] |= (uint64_t)(r & 0xFFFFu) << (16 * (k & 3));
  }
  uint64_t* const rec = t64 + kSeekHeaderBytes / 8 + g * (kSeekRecordBytes / 8);
  rec[0] = P.chunk_bit[g];
  rec[1] = w[0];
  rec[2] = w[1];
  if (bad) latch_status(P.status, GHF_E_CORRUPT);  // a side-car whose segment ends do not grow: not one of ours
}

// A lane's cursor over the stream in global memory: big-endian words in order, from whole 16-byte vectors (the stream's
// last, incomplete one: byte loads; behind the stream: zeros -- no address outside stream[0 .. bytes) is ever formed into
// a load, whatever the start bit).  The vector behind the current one is always in flight.
struct SeekCursor {
  const uint8_t* s;
  uint64_t bytes, full_bytes;
  uint64_t vnext;  // the next vector to request
  uint4 cur, nxt;
  uint32_t left;   // words of `cur` not yet handed out
  uint64_t W;
  uint32_t nextw, o;
  __device__ __forceinline__ uint4 load(uint64_t v) const {
    const uint64_t b = v << 4;
    uint4 r = make_uint4(0, 0, 0, 0);
    if (b + 16 <= full_bytes) {
      r = *reinterpret_cast<const uint4*>(s + b);
      r = make_uint4(bswap32(r.x), bswap32(r.y), bswap32(r.z), bswap32(r.w));
    } else if (b < bytes) {
      uint32_t q[4] = {0, 0, 0, 0};
#pragma unroll
      for (int j = 0; j < 16; ++j)
        if (b + j < bytes) q[j >> 2] |= (uint32_t)s[b + j] << (24 - 8 * (j & 3));
      r = make_uint4(q[0], q[1], q[2], q[3]);
    }
    return r;
  }
  // the same vector as it stands in memory (the step walk swaps a word where it takes it: a swap behind the load would make
  // the wave wait for the vector where it asked for it)
  __device__ __forceinline__ uint4 load_raw(uint64_t v) const {
    const uint64_t b = v << 4;
    uint4 r = make_uint4(0, 0, 0, 0);
    if (b + 16 <= full_bytes) {
      r = *reinterpret_cast<const uint4*>(s + b);
    } else if (b < bytes) {
      uint32_t q[4] = {0, 0, 0, 0};
#pragma unroll
      for (int j = 0; j < 16; ++j)
        if (b + j < bytes) q[j >> 2] |= (uint32_t)s[b + j] << (8 * (j & 3));
      r = make_uint4(q[0], q[1], q[2], q[3]);
    }
    return r;
  }
  __device__ __forceinline__ uint32_t word() {
    if (left == 0) {
      cur = nxt;
      nxt = load(vnext);
      ++vnext;
      left = 4;
    }
    const uint32_t w = cur.x;
    cur.x = cur.y;
    cur.y = cur.z;
    cur.z = cur.w;
    --left;
    return w;
  }
  // bit <= 8 * bytes (the callers check)
  __device__ __forceinline__ void open(const uint8_t* stream, uint64_t stream_bytes, uint64_t bit) {
    s = stream;
    bytes = stream_bytes;
    full_bytes = stream_bytes & ~15ull;
    const uint64_t widx = bit >> 5;
    const uint64_t v = widx >> 2;
    cur = load(v);
    nxt = load(v + 1);
    vnext = v + 2;
    left = 4;
    for (uint32_t k = (uint32_t)(widx & 3u); k; --k) (void)word();
    const uint32_t w0 = word(), w1 = word();
    W = win_open(w0, w1);
    nextw = word();
    o = (uint32_t)(bit & 31u);
  }
  // entry (symbol | length << 8 | kEntEnd) of the code at the cursor; the cursor moves behind it
  __device__ __forceinline__ uint32_t step(const DecLds& L, const DecLut& T, int lut_bits, int max_len) {
    while (o >= 32u) {  // (a code of up to 64 bits moves the cursor by up to two words)
      win_shift(W, nextw, o);
      nextw = word();
    }
    uint32_t ent = dec_lookup(T, win_peek(W, o));
    if (ent & kEntNone) ent = dec_long_entry_at(L, W, nextw, o, lut_bits, max_len);
    o += (ent >> 8) & 0xFFu;
    return ent;
  }
};

constexpr int kSeekThreads = 1024;

// One lane per run of 512 symbols.  The lane starts at start_bit + (the lengths of the runs in front of it), decodes code
// lengths only, writes the end of each of its eight segments relative to the block, and must land exactly on the run's
// recorded end; lane 0 of a block writes chunk_bit and checks that the block's runs add up to the next record's start.
// A table that fails either test, or names a bit outside the stream, latches GHF_E_CORRUPT.  Touches neither the ticket
// counters nor `done` of DecTables.
// r: the run, counted from the table's first block; L: the tables of P.dt, loaded by the caller.
//
// kRounds = false is k_seek_expand's walk: a SeekCursor per lane.  Its refills are data dependent, so in every step some lane
// of the wave refills, and the wave waits for a vector load in every step: measured, 0.37 us per symbol, 0.19 ms for a run
// whatever the range.  kRounds = true (k_seek_expand_planes; codes of up to 32 bits) walks in ROUNDS instead: all lanes
// load their next vector in the same instruction, one round ahead, and a lane then decodes whatever starts inside the words
// it has, with no memory access inside a round.  W holds two stream words and `o` the offset of the next code from W's top;
// feeding a word drops W's upper word.  The walk opens with o = 64 + (the start bit's offset in its vector): the code "starts"
// that far behind two words that are not there yet, and the first words fed only bring o down.
//
// kSteps (k_seek_expand_streams; codes of up to 32 bits) walks in STEPS.  In a round every lane decodes the codes that start in
// ITS word while the wave waits for the lane with the most of them, word after word: on streams whose code lengths vary --
// the masks and values of sparse planes: 1 to 19 bits -- a wave made 1400 passes through the decode chain for its 512 symbols
// (measured: 1035 cycles per symbol on the values of a bf16 delta plane, 357 on a mask of 1-bit codes; the loads and the
// miss path together were under 3 % of it).  Here a pass of the wave is one symbol of every lane, 512 passes for a run,
// whatever the lengths.  A lane owns three vectors: `cur`, which it takes words from, `nxt` behind it and `fut` in flight.
// Every T = 128 / max_len - 1 symbols -- no lane can use up more than one vector in between -- the wave stops at a refill point:
// it waits for the vectors requested at the last one, and a lane whose `nxt` has moved up gets `fut` and requests the next.
// Between two refill points there is no memory access but the side-car's own stores.
template <bool kRounds, bool kSteps = false>
__device__ __forceinline__ void seek_expand_run(const SeekExpandParams& P, const DecLds& L, int lut_bits, int max_len, int pair_bits,
                                                uint64_t r, int tid) {
  const uint64_t g = r >> 3;
  const uint32_t k = (uint32_t)r & 7u;
  if (g >= P.g1 || g >= P.n_blocks) return;
  const uint64_t* const rec = reinterpret_cast<const uint64_t*>(P.records) + g * (kSeekRecordBytes / 8);
  const uint64_t start = rec[0];
  const uint64_t w0 = rec[1], w1 = rec[2];
  const uint64_t next_start = (g + 1 < P.n_blocks) ? rec[3] : 0;
  uint32_t before = 0, mine = 0, total = 0;
#pragma unroll
  for (int j = 0; j < kRunsPerBlock; ++j) {
    const uint32_t b = (uint32_t)(((j < 4 ? w0 : w1) >> (16 * (j & 3))) & 0xFFFFu);
    before += (uint32_t)j < k ? b : 0u;
    mine = (uint32_t)j == k ? b : mine;
    total += b;
  }
  const uint64_t end_bit = P.stream_bytes * 8;
  bool bad = start > end_bit || total > end_bit - start;
  if (k == 0) {
    P.chunk_bit[g - P.g0] = bad ? 0ull : start;
    if (g + 1 < P.n_blocks && next_start - start != (uint64_t)total) bad = true;
  }
  const uint64_t sym0 = g * kBlockSymbols + (uint64_t)k * kRunSymbols;
  const uint32_t nsym = sym0 >= P.n_symbols ? 0u : (P.n_symbols - sym0 >= (uint64_t)kRunSymbols ? (uint32_t)kRunSymbols : (uint32_t)(P.n_symbols - sym0));
  uint32_t* const seg_out = P.seg_bit + (g - P.g0) * (kBlockSymbols / kSegSymbols) + k * kRunSegs;
  if (bad || nsym == 0) {
    if (nsym == 0 && mine != 0) bad = true;  // runs behind the stream's last symbol are empty
    for (uint32_t j = 0; j * kSegSymbols < nsym; ++j) seg_out[j] = 0;
    if (bad) latch_status(P.status, GHF_E_CORRUPT);
    return;
  }
  const DecLut T = dec_lut1(L.lut, lut_bits, pair_bits, tid & 63);
  SeekCursor c;
  uint32_t used = 0, acc = 0;
  if (kSteps && max_len <= 32) {
    const uint64_t B = start + before;
    c.s = P.stream;
    c.bytes = P.stream_bytes;
    c.full_bytes = P.stream_bytes & ~15ull;
    uint64_t v = B >> 7;
    uint4 cur = c.load_raw(v), nxt = c.load_raw(v + 1), fut = c.load_raw(v + 2);
    v += 3;
    uint32_t left = 4;       // words of `cur` not yet taken
    bool have_nxt = true;    // false: nxt has moved up into cur and fut has not yet moved up into nxt
    auto take = [&]() -> uint32_t {  // the stream's next word
      if (left == 0) {       // (have_nxt holds here: see T)
        cur = nxt;
        have_nxt = false;
        left = 4;
      }
      const uint32_t w = bswap32(cur.x);
      cur.x = cur.y;
      cur.y = cur.z;
      cur.z = cur.w;
      --left;
      return w;
    };
    for (uint32_t k0 = (uint32_t)(B >> 5) & 3u; k0; --k0) (void)take();
    const uint32_t w0 = take(), w1 = take();
    uint64_t W = win_open(w0, w1);
    uint32_t o = (uint32_t)(B & 31u), done = 0;
    // Behind a refill point nxt is whole: a lane holds at least four words it has not taken.  A word is taken in front of a
    // symbol, when o >= 32; o is at most 31 + max_len where the span begins, so T symbols take at most
    // (31 + (T + 1) max_len) / 32 words: four with T = 128 / max_len - 1.  Four words move nxt up at most once.
    const uint32_t span = 128u / (uint32_t)max_len - 1u;  // T: 3 (max_len 32) .. 127
#pragma unroll 1
    while (__any(done < nsym)) {
      if (!have_nxt) {  // fut was requested at the last refill point (or in front of the walk): this is where the wave waits for it
        nxt = fut;
        have_nxt = true;
        fut = done < nsym ? c.load_raw(v) : make_uint4(0, 0, 0, 0);
        ++v;
      }
#pragma unroll 1
      for (uint32_t t = 0; t < span; ++t) {
        if (done < nsym) {
          if (o >= 32u) {
            W = (W << 32) | take();
            o -= 32u;
          }
          const uint32_t hi = win_peek(W, o);
          uint32_t ent = dec_lookup(T, hi);
          if (ent & kEntNone) ent = dec_long_entry(L, hi, lut_bits, max_len);
          const uint32_t len = (ent >> 8) & 0xFFu;
          acc |= ent;
          used += len;
          o += len;
          ++done;
          if ((done & (uint32_t)(kSegSymbols - 1)) == 0 || done == nsym) seg_out[(done - 1) / kSegSymbols] = before + used;
        }
      }
    }
  } else if (kRounds && max_len <= 32) {
    const uint64_t B = start + before;
    c.s = P.stream;
    c.bytes = P.stream_bytes;
    c.full_bytes = P.stream_bytes & ~15ull;
    uint64_t v = B >> 7;
    uint4 cur = c.load(v), nxt = c.load(v + 1);
    v += 2;
    uint64_t W = 0;
    uint32_t o = 64u + (uint32_t)(B & 127u), done = 0;
    auto feed = [&](uint32_t nw) {
      while (o < 32u && done < nsym) {
        const uint32_t hi = win_peek(W, o);
        uint32_t ent = dec_lookup(T, hi);
        if (ent & kEntNone) ent = dec_long_entry(L, hi, lut_bits, max_len);
        const uint32_t len = (ent >> 8) & 0xFFu;
        acc |= ent;
        used += len;
        o += len;
        ++done;
        if ((done & (uint32_t)(kSegSymbols - 1)) == 0 || done == nsym) seg_out[(done - 1) / kSegSymbols] = before + used;
      }
      if (o >= 32u) {
        W = (W << 32) | nw;
        o -= 32u;
      }
    };
#pragma unroll 1
    while (__any(done < nsym)) {
      const uint4 x = cur;
      cur = nxt;
      nxt = done < nsym ? c.load(v) : make_uint4(0, 0, 0, 0);
      ++v;
      feed(x.x);
      feed(x.y);
      feed(x.z);
      feed(x.w);
    }
  } else {
    c.open(P.stream, P.stream_bytes, start + before);
#pragma unroll 1
    for (uint32_t done = 0; done < nsym;) {
      const uint32_t stop = done + (uint32_t)kSegSymbols < nsym ? done + (uint32_t)kSegSymbols : nsym;
#pragma unroll 1
      for (; done < stop; ++done) {
        const uint32_t ent = c.step(L, T, lut_bits, max_len);
        acc |= ent;
        used += (ent >> 8) & 0xFFu;
      }
      seg_out[(stop - 1) / kSegSymbols] = before + used;
    }
  }
  if (used != mine || (acc & (kEntEnd | kEntNone))) latch_status(P.status, GHF_E_CORRUPT);
}

__global__ __launch_bounds__(kSeekThreads) void k_seek_expand(SeekExpandParams P) {
  __shared__ DecLds L;
  const int tid = threadIdx.x;
  if (tid == 0) L.status0 = *P.status;
  const int lut_bits = P.dt->lut_bits, max_len = P.dt->max_len, pair_bits = P.dt->pair_bits;
  dec_lds_load(L, P.dt, tid, kSeekThreads);
  __syncthreads();
  if (L.status0 != 0) return;
  seek_expand_run<false>(P, L, lut_bits, max_len, pair_bits, P.g0 * kRunsPerBlock + (uint64_t)blockIdx.x * kSeekThreads + (uint32_t)tid, tid);
}

// The same for the covered blocks of up to GHF_PLANES_MAX streams in ONE launch (ghf_decode_planes_range; DESIGN.md
// section 17): blockIdx.y names the stream, every stream has its own tables, and all of them cover the blocks [g0, g1) of
// streams of one n_symbols.  A lane's walk over its 512 symbols is serial, so the launch cannot take less than one walk;
// what it can avoid is paying that once per plane, and crowding sixteen waves onto one CU when the range is small: the
// workgroup is as narrow as the launch's waves allow (launch_seek_expand_planes), down to one wave.
__global__ __launch_bounds__(kSeekThreads) void k_seek_expand_planes(SeekExpandPlanesParams A) {
  __shared__ DecLds L;
  const SeekExpandParams& P = A.plane[blockIdx.y];
  const int tid = threadIdx.x;
  if (tid == 0) L.status0 = *P.status;
  const int lut_bits = P.dt->lut_bits, max_len = P.dt->max_len, pair_bits = P.dt->pair_bits;
  dec_lds_load(L, P.dt, tid, (int)blockDim.x);
  __syncthreads();
  if (L.status0 != 0) return;
  seek_expand_run<true>(P, L, lut_bits, max_len, pair_bits, P.g0 * kRunsPerBlock + (uint64_t)blockIdx.x * blockDim.x + (uint32_t)tid, tid);
}

// The same for streams that have nothing in common (ghf_decode_planes_sparse_range): the planes, masks
// and values of one tensor, every one with its own n_symbols, its own tables and its own blocks [g0, g1).  blockIdx.y names the
// stream and grid.x is sized by the widest one: a workgroup beyond its stream's own runs -- and every workgroup of a slot with
// g1 == g0, whose other fields are then not looked at -- leaves before it loads a table.
__global__ __launch_bounds__(kSeekThreads) void k_seek_expand_streams(SeekExpandStreamsParams A) {
  __shared__ DecLds L;
  const SeekExpandParams& P = A.stream[blockIdx.y];
  if ((uint64_t)blockIdx.x * blockDim.x >= (P.g1 - P.g0) * kRunsPerBlock) return;
  const int tid = threadIdx.x;
  if (tid == 0) L.status0 = *P.status;
  const int lut_bits = P.dt->lut_bits, max_len = P.dt->max_len, pair_bits = P.dt->pair_bits;
  dec_lds_load(L, P.dt, tid, (int)blockDim.x);
  __syncthreads();
  if (L.status0 != 0) return;
  seek_expand_run<true, true>(P, L, lut_bits, max_len, pair_bits, P.g0 * kRunsPerBlock + (uint64_t)blockIdx.x * blockDim.x + (uint32_t)tid, tid);
}

// The head of a range that does not begin on a block boundary: one wave, one lane per segment of the block, same tables;
// a lane decodes its segment from the side-car's start and stores the symbols of [lo, hi) only.  A segment that is decoded
// to its end is checked against the side-car like K7 does.
__global__ __launch_bounds__(64) void k_decode_head(DecHeadParams P) {
  __shared__ DecLds L;
  const int lane = threadIdx.x;
  if (lane == 0) L.status0 = *P.status;
  const int lut_bits = P.dt->lut_bits, max_len = P.dt->max_len, pair_bits = P.dt->pair_bits;
  dec_lds_load(L, P.dt, lane, 64);
  __syncthreads();
  if (L.status0 != 0) return;
  const uint64_t a = P.blk_sym0 + (uint64_t)lane * kSegSymbols;  // my segment: symbols [a, b)
  if (a >= P.n_symbols) return;
  const uint64_t b = P.n_symbols - a >= (uint64_t)kSegSymbols ? a + kSegSymbols : P.n_symbols;
  if (b <= P.lo || a >= P.hi) return;
  const uint64_t B0 = P.chunk_bit[0];
  const uint32_t start = lane ? P.seg_bit[lane - 1] : 0u;
  const uint32_t end = P.seg_bit[lane];
  const uint64_t end_bit = P.stream_bytes * 8;
  if (end < start || B0 > end_bit || (uint64_t)end > end_bit - B0) {
    latch_status(P.status, GHF_E_CORRUPT);
    return;
  }
  const DecLut T = dec_lut1(L.lut, lut_bits, pair_bits, lane);
  SeekCursor c;
  c.open(P.stream, P.stream_bytes, B0 + start);
  const uint64_t stop = b < P.hi ? b : P.hi;
  uint32_t used = 0, acc = 0;
#pragma unroll 1
  for (uint64_t i = a; i < stop; ++i) {
    const uint32_t ent = c.step(L, T, lut_bits, max_len);
    acc |= ent;
    used += (ent >> 8) & 0xFFu;
    if (i >= P.lo) P.out[i - P.lo] = (uint8_t)ent;
  }
  const bool whole = stop == b && b < P.n_symbols;  // (the stream's last segment: what follows it is K7's business)
  if ((whole && used != end - start) || (acc & (kEntEnd | kEntNone))) latch_status(P.status, GHF_E_CORRUPT);
}

void launch_seek_pack(const SeekPackParams& p, hipStream_t s) {
  const uint64_t blocks = (p.n_blocks + 255) / 256;
  hipLaunchKernelGGL(k_seek_pack, dim3((uint32_t)(blocks ? blocks : 1)), dim3(256), 0, s, p);
}
void launch_seek_expand(const SeekExpandParams& p, hipStream_t s) {
  if (p.g1 <= p.g0) return;
  const uint64_t lanes = (p.g1 - p.g0) * kRunsPerBlock;
  hipLaunchKernelGGL(k_seek_expand, dim3((uint32_t)((lanes + kSeekThreads - 1) / kSeekThreads)), dim3(kSeekThreads), 0, s, p);
}
// one resident round where the range allows it: two workgroups of these tables fit on a CU, so up to 512 workgroups, each
// of as few waves (1 .. 16) as that takes
void launch_seek_expand_planes(const SeekExpandPlanesParams& a, uint32_t planes, hipStream_t s) {
  const SeekExpandParams& p = a.plane[0];
  if (p.g1 <= p.g0 || planes == 0) return;
  const uint64_t lanes = (p.g1 - p.g0) * kRunsPerBlock, waves = (lanes + 63) / 64 * planes;
  const uint64_t per = (waves + 511) / 512;
  const uint32_t threads = 64u * (uint32_t)(per < 1 ? 1 : per > kSeekThreads / 64 ? kSeekThreads / 64 : per);
  hipLaunchKernelGGL(k_seek_expand_planes, dim3((uint32_t)((lanes + threads - 1) / threads), planes), dim3(threads), 0, s, a);
}
// the same rule with the streams' own widths: the waves of all streams decide how narrow a workgroup may be, the widest
// stream decides grid.x
void launch_seek_expand_streams(const SeekExpandStreamsParams& a, uint32_t streams, hipStream_t s) {
  uint64_t widest = 0, waves = 0;
  for (uint32_t j = 0; j < streams; ++j) {
    const SeekExpandParams& p = a.stream[j];
    const uint64_t lanes = p.g1 > p.g0 ? (p.g1 - p.g0) * kRunsPerBlock : 0;
    widest = lanes > widest ? lanes : widest;
    waves += (lanes + 63) / 64;
  }
  if (widest == 0) return;
  const uint64_t per = (waves + 511) / 512;
  const uint32_t threads = 64u * (uint32_t)(per < 1 ? 1 : per > kSeekThreads / 64 ? kSeekThreads / 64 : per);
  hipLaunchKernelGGL(k_seek_expand_streams, dim3((uint32_t)((widest + threads - 1) / threads), streams), dim3(threads), 0, s, a);
}
void launch_decode_head(const DecHeadParams& p, hipStream_t s) {
  if (p.hi <= p.lo) return;
  hipLaunchKernelGGL(k_decode_head, dim3(1), dim3(64), 0, s, p);
}

}  // namespace ghf
