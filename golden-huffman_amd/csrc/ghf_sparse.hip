// golden-huffman_amd/csrc/ghf_sparse.hip -- zero-suppressed byte strings.
// split: x[0 .. n) -> mask (bit k & 7 of mask[k >> 3] = (x[k] != 0), LSB first, pad bits 0) and vals = x[x != 0] in order.
// merge: the inverse.  Both need, for every tile of x, where its non-zero bytes start in vals.  That offset is made by
// THREE LAUNCHES on the stream and by nothing else: no kernel here waits for a store of another workgroup.
//   1. count:  every workgroup counts the non-zero bytes of its slab of tiles -> counts[group]   (split: and writes the mask;
//              merge: popcounts of the mask, and the pad bits are checked)
//   2. scan:   one workgroup: offs[group] = sum of the counts in front of it, offs[groups] = the total; the total is held
//              against vals_cap (split: GHF_E_CAP) or n_vals (merge: GHF_E_CORRUPT)
//   3. move:   every workgroup walks its slab again, tile by tile, carrying its own running offset from offs[group]
// One wave = one workgroup, a tile = 64 lanes x 4 vectors of 16 bytes = kSparseTile bytes of x, lane l on vector 64 j + l
// (the access shape of ghf_planes.hip: 16 bytes per lane, consecutive lanes on consecutive vectors, the non-temporal hint,
// four loads in flight before the first use, one resident round of kSparseGroups workgroups with a contiguous slab each).
// The compacted side goes through the wave's LDS tile: the tile's values stand in it at the byte phase they have in vals
// (LDS byte i <-> vals byte (base & ~15) + i), so that every 16-byte vector of vals that lies wholly inside the tile's
// run is one aligned global vector store (load); only the run's ragged head and tail are stored byte by byte.  Inside the tile
// the split deals a vector's non-zero bytes into the LDS with one byte store per set mask bit; the merge takes a vector's
// values out of it as one 16-byte window and deals them out in registers.
#include "ghf_device.h"

namespace ghf {

namespace {

constexpr int kVec = 4;                                       // 16-byte vectors per lane and tile
constexpr uint32_t kTileVecs = kWave * kVec;                  // 256
constexpr uint32_t kMaskTileBytes = kSparseTile / 8;          // 512
constexpr uint32_t kStageVecs = kTileVecs + 2;                // a run of <= 4096 bytes at any phase: <= 257 vectors (+1 spare)
static_assert(kTileVecs * 16 == kSparseTile, "the tile the host counts with");
static_assert(kStageVecs * 16 == kSparseLdsBytes, "the LDS budget of DESIGN.md section 20");

__device__ __forceinline__ uint4 ld16(const void* p) { return load_stream(p); }
__device__ __forceinline__ void st16(void* p, const uint4& v) { store_stream(p, v); }

// the slab of tiles of this workgroup; the last tile of the string may be a partial one
struct Slab {
  uint64_t lo, end;
};
__device__ __forceinline__ Slab slab_of(uint64_t n) {
  const uint64_t nt = (n + kSparseTile - 1) / kSparseTile, per = (nt + gridDim.x - 1) / gridDim.x;
  const uint64_t lo = (uint64_t)blockIdx.x * per;
  return {lo < nt ? lo : nt, lo + per < nt ? lo + per : nt};
}

// bit q = (byte q of d != 0)
__device__ __forceinline__ uint32_t nz4(uint32_t d) {
  const uint32_t hi = (((d & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | d) & 0x80808080u;  // bit 7 of every non-zero byte
  return ((hi >> 7) * 0x00204081u >> 21) & 15u;                              // bits 0, 8, 16, 24 -> bits 21 .. 24
}
__device__ __forceinline__ uint32_t nz16(const uint4& x) { return nz4(x.x) | nz4(x.y) << 4 | nz4(x.z) << 8 | nz4(x.w) << 12; }

// the first `keep` bytes of x, zeros behind them (keep >= 16: x)
__device__ __forceinline__ uint32_t trim4(uint32_t d, int keep) { return keep >= 4 ? d : keep <= 0 ? 0u : d & (0xFFFFFFFFu >> (32 - 8 * keep)); }
__device__ __forceinline__ uint4 trim16(const uint4& x, int keep) {
  return make_uint4(trim4(x.x, keep), trim4(x.y, keep - 4), trim4(x.z, keep - 8), trim4(x.w, keep - 12));
}

__device__ __forceinline__ uint32_t byte_of(const uint4& x, uint32_t k) {
  const uint64_t q = (k & 8u) ? (uint64_t)x.w << 32 | x.z : (uint64_t)x.y << 32 | x.x;  // selects, never an indexed array
  return (uint32_t)(q >> (8 * (k & 7u))) & 0xFFu;
}
__device__ __forceinline__ void put_byte(uint4& x, uint32_t k, uint32_t b) {
  const uint32_t w = k >> 2, v = b << (8 * (k & 3u));
  x.x |= w == 0 ? v : 0u;
  x.y |= w == 1 ? v : 0u;
  x.z |= w == 2 ? v : 0u;
  x.w |= w == 3 ? v : 0u;
}

// the tile's kVec vectors of this lane; `valid` (wave-uniform) = bytes of the tile inside the string.  A vector that
// holds the last valid byte is loaded whole and trimmed, one behind it is not loaded
__device__ __forceinline__ void load_tile(const uint8_t* src, uint32_t valid, uint32_t lane, uint4 (&x)[kVec]) {
  if (valid == kSparseTile) {
#pragma unroll
    for (int j = 0; j < kVec; ++j) x[j] = ld16(src + (j * kWave + lane) * 16);
  } else {
#pragma unroll
    for (int j = 0; j < kVec; ++j) {
      const uint32_t at = (j * kWave + lane) * 16;
      x[j] = make_uint4(0, 0, 0, 0);
      if (at < valid) x[j] = trim16(ld16(src + at), (int)(valid - at));
    }
  }
}

// the lane's four masks -> where the values of its vector j start in the tile's run (off[j]); -> the run's length
__device__ __forceinline__ uint32_t tile_offsets(const uint32_t (&m)[kVec], uint32_t (&off)[kVec]) {
  uint32_t run = 0;
#pragma unroll
  for (int j = 0; j < kVec; ++j) {
    const uint32_t c = __builtin_popcount(m[j]), incl = wave_incl_scan_u32(c);
    off[j] = run + incl - c;
    run += wave_last_u32(incl);
  }
  return run;
}

// sum of v over the wave, in lane 0 (once per launch: through the LDS)
__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v, uint64_t* lds, uint32_t lane) {
  lds[lane] = v;
  wave_sync();
  uint64_t s = 0;
  if (lane == 0)
    for (int i = 0; i < kWave; ++i) s += lds[i];
  wave_sync();
  return s;
}

}  // namespace

// ---- split, launch 1: the mask, and the slab's count -------------------------------------------------------------------
__global__ __launch_bounds__(kWave) void k_sparse_split_count(const uint8_t* __restrict__ in, uint64_t n, uint8_t* __restrict__ mask,
                                                              uint64_t* __restrict__ counts) {
  __shared__ uint4 lds[kMaskTileBytes / 16];  // the tile's mask; at the end the 64 partial counts
  uint16_t* mtile = reinterpret_cast<uint16_t*>(lds);
  const uint32_t lane = threadIdx.x;
  const Slab s = slab_of(n);
  uint64_t mine = 0;
  for (uint64_t t = s.lo; t < s.end; ++t) {
    const uint64_t left = n - t * kSparseTile;
    const uint32_t valid = left < kSparseTile ? (uint32_t)left : kSparseTile;
    uint4 x[kVec];
    load_tile(in + t * kSparseTile, valid, lane, x);
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < kVec; ++j) {
      const uint32_t m = nz16(x[j]);
      c += __builtin_popcount(m);
      mtile[j * kWave + lane] = (uint16_t)m;
    }
    mine += c;
    wave_sync();
    uint8_t* dst = mask + t * kMaskTileBytes;
    const uint32_t mbytes = (valid + 7) / 8, at = lane * 16;
    if (at + 16 <= mbytes) {
      st16(dst + at, lds[lane]);
    } else if (at < mbytes) {  // the string's last mask bytes
      const uint8_t* b = reinterpret_cast<const uint8_t*>(lds);
      for (uint32_t i = at; i < mbytes; ++i) dst[i] = b[i];
    }
    wave_sync();
  }
  const uint64_t total = wave_sum_u64(mine, reinterpret_cast<uint64_t*>(lds), lane);
  if (lane == 0) counts[blockIdx.x] = total;
}

// ---- merge, launch 1: the popcount of the slab's mask bytes; a set pad bit latches GHF_E_CORRUPT ----------------------------
__global__ __launch_bounds__(kWave) void k_sparse_merge_count(const uint8_t* __restrict__ mask, uint64_t n, uint64_t* __restrict__ counts,
                                                              int* __restrict__ status) {
  __shared__ uint64_t lds[kWave];
  if (__builtin_amdgcn_readfirstlane(*status) != 0) return;
  const uint32_t lane = threadIdx.x;
  const Slab s = slab_of(n);
  const uint64_t mb = (n + 7) / 8;
  const uint64_t lo = s.lo * kMaskTileBytes, hi = s.end * kMaskTileBytes < mb ? s.end * kMaskTileBytes : mb;  // lo is a multiple of 16
  const uint64_t nv = hi > lo ? (hi - lo + 15) / 16 : 0;
  uint64_t mine = 0;
  for (uint64_t v0 = 0; v0 < nv; v0 += kWave * kVec) {
    uint4 x[kVec];
#pragma unroll
    for (int j = 0; j < kVec; ++j) {
      const uint64_t v = v0 + j * kWave + lane;
      x[j] = make_uint4(0, 0, 0, 0);
      if (v < nv) x[j] = ld16(mask + lo + v * 16);
    }
#pragma unroll
    for (int j = 0; j < kVec; ++j) {
      const uint64_t v = v0 + j * kWave + lane;
      if (v < nv && hi - lo - v * 16 < 16) x[j] = trim16(x[j], (int)(hi - lo - v * 16));  // behind the last mask byte: not ours
      mine += __builtin_popcount(x[j].x) + __builtin_popcount(x[j].y) + __builtin_popcount(x[j].z) + __builtin_popcount(x[j].w);
    }
  }
  if (blockIdx.x == gridDim.x - 1 && lane == 0 && (n & 7u) && (mask[mb - 1] >> (n & 7u)) != 0) latch_status(status, GHF_E_CORRUPT);
  const uint64_t total = wave_sum_u64(mine, lds, lane);
  if (lane == 0) counts[blockIdx.x] = total;
}

// ---- launch 2: offs[g] = counts[0] + .. + counts[g - 1], offs[groups] = the total.  One workgroup ---------------------------
// split (d_n_vals != null): *d_n_vals <- the total; a total above `limit` (= vals_cap) latches GHF_E_CAP.
// merge (d_n_vals == null): a total other than `limit` (= n_vals) latches GHF_E_CORRUPT.
constexpr int kScanThreads = 256;
constexpr int kScanPer = kSparseGroups / kScanThreads;
__global__ __launch_bounds__(kScanThreads) void k_sparse_scan(const uint64_t* __restrict__ counts, uint32_t groups, uint64_t* __restrict__ offs,
                                                              uint64_t limit, uint64_t* __restrict__ d_n_vals, int* __restrict__ status) {
  __shared__ uint64_t part[kScanThreads];
  const uint32_t tid = threadIdx.x;
  uint64_t c[kScanPer], sum = 0;
#pragma unroll
  for (int i = 0; i < kScanPer; ++i) {
    const uint32_t g = tid * kScanPer + i;
    c[i] = g < groups ? counts[g] : 0;
    sum += c[i];
  }
  part[tid] = sum;
  __syncthreads();
  for (uint32_t d = 1; d < kScanThreads; d <<= 1) {
    const uint64_t v = tid >= d ? part[tid - d] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  uint64_t run = part[tid] - sum;
#pragma unroll
  for (int i = 0; i < kScanPer; ++i) {
    const uint32_t g = tid * kScanPer + i;
    if (g < groups) offs[g] = run;
    run += c[i];
  }
  if (tid == kScanThreads - 1) {
    const uint64_t total = part[tid];
    offs[groups] = total;
    if (d_n_vals) {
      *d_n_vals = total;
      if (total > limit) latch_status(status, GHF_E_CAP);
    } else if (total != limit) {
      latch_status(status, GHF_E_CORRUPT);
    }
  }
}

// ---- split, launch 3: the compaction ------------------------------------------------------------------------------------------
// a total above vals_cap: nothing is stored (the scan has latched GHF_E_CAP)
__global__ __launch_bounds__(kWave) void k_sparse_split_move(const uint8_t* __restrict__ in, uint64_t n, uint8_t* __restrict__ vals,
                                                             uint64_t vals_cap, const uint64_t* __restrict__ offs) {
  __shared__ uint4 stage[kStageVecs];
  uint8_t* sb = reinterpret_cast<uint8_t*>(stage);
  if (offs[gridDim.x] > vals_cap) return;
  const uint32_t lane = threadIdx.x;
  const Slab s = slab_of(n);
  uint64_t base = offs[blockIdx.x];
  for (uint64_t t = s.lo; t < s.end; ++t) {
    const uint64_t left = n - t * kSparseTile;
    const uint32_t valid = left < kSparseTile ? (uint32_t)left : kSparseTile;
    uint4 x[kVec];
    load_tile(in + t * kSparseTile, valid, lane, x);
    uint32_t m[kVec], off[kVec];
#pragma unroll
    for (int j = 0; j < kVec; ++j) m[j] = nz16(x[j]);
    const uint32_t run = tile_offsets(m, off);
    if (run == 0) continue;
    const uint32_t skew = (uint32_t)base & 15u, end = skew + run;  // end <= 15 + 4096
#pragma unroll
    for (int j = 0; j < kVec; ++j) {
      uint32_t o = skew + off[j];
      for (uint32_t mm = m[j]; mm; mm &= mm - 1) sb[o++] = (uint8_t)byte_of(x[j], __builtin_ctz(mm));
    }
    wave_sync();
    uint8_t* dst = vals + (base - skew);  // 16-byte aligned; LDS byte i <-> dst[i]
    const uint32_t v0 = skew ? 1u : 0u, v1 = end >> 4;  // the vectors [v0, v1) lie wholly inside the run
    for (uint32_t v = v0 + lane; v < v1; v += kWave) st16(dst + v * 16, stage[v]);
    if (lane < 16) {  // the ragged head: [skew, min(16, end))
      if (skew && lane >= skew && lane < end) dst[lane] = sb[lane];
    } else if (lane < 32) {  // the ragged tail: [16 v1, end), unless the head was that vector
      const uint32_t i = v1 * 16 + (lane - 16);
      if ((v1 > 0 || skew == 0) && i < end) dst[i] = sb[i];
    }
    wave_sync();
    base += run;
  }
}

// ---- merge, launch 3: the expansion -----------------------------------------------------------------------------------------------
// the lane's four mask words of tile t: vector 64 j + l of the tile takes mask bytes 2 (64 j + l) and the next
__device__ __forceinline__ void load_masks(const uint8_t* __restrict__ mask, uint64_t n, uint64_t t, uint32_t lane, uint32_t (&m)[kVec]) {
  const uint64_t left = n - t * kSparseTile;
  const uint8_t* msrc = mask + t * kMaskTileBytes;
  if (left >= kSparseTile) {
#pragma unroll
    for (int j = 0; j < kVec; ++j) m[j] = reinterpret_cast<const uint16_t*>(msrc)[j * kWave + lane];
  } else {  // the string's last mask bytes, one by one: nothing behind mask[(n + 7) / 8) is read
    const uint32_t mbytes = ((uint32_t)left + 7) / 8;
#pragma unroll
    for (int j = 0; j < kVec; ++j) {
      const uint32_t at = (j * kWave + lane) * 2;
      m[j] = (at < mbytes ? msrc[at] : 0u) | (at + 1 < mbytes ? (uint32_t)msrc[at + 1] << 8 : 0u);
    }
  }
}

// LDS bytes [o, o + 16) as a vector: the five aligned dwords that hold them, funnelled by the byte part of o
__device__ __forceinline__ uint4 window16(const uint32_t* lds32, uint32_t o) {
  const uint32_t a = o >> 2, b = o & 3u;
  const uint32_t d0 = lds32[a], d1 = lds32[a + 1], d2 = lds32[a + 2], d3 = lds32[a + 3], d4 = lds32[a + 4];
  return make_uint4(__builtin_amdgcn_alignbyte(d1, d0, b), __builtin_amdgcn_alignbyte(d2, d1, b), __builtin_amdgcn_alignbyte(d3, d2, b),
                    __builtin_amdgcn_alignbyte(d4, d3, b));
}

// a launch that finds the status word non-zero stores nothing: that is also how a count that does not match n_vals (the scan)
// and a set pad bit (the count) keep every byte of `out` as it was.  The masks of the next tile are requested behind the
// values of this one, so that one memory round trip stands in front of a tile's stores, not two.  A lane takes the (up to
// 16) values of a vector out of the LDS tile as one 16-byte window and deals them out in registers.
// `skip`: where the string's first value stands in vals (k_sparse_merge_move: 0; k_sparse_merge_move_at: the caller's
// vals_skip).  It is one more term of the workgroup's base offset and of nothing else: the tile stands in the LDS at the phase
// (skip + its offset) & 15, which the 4128 bytes cover like any other.
__device__ __forceinline__ void sparse_merge_move(uint4 (&stage)[kStageVecs], const uint8_t* __restrict__ mask, const uint8_t* __restrict__ vals,
                                                  uint64_t skip, uint64_t n, uint8_t* __restrict__ out, const uint64_t* __restrict__ offs,
                                                  const int* __restrict__ status) {
  const uint32_t* s32 = reinterpret_cast<const uint32_t*>(stage);
  if (__builtin_amdgcn_readfirstlane(*status) != 0) return;
  const uint32_t lane = threadIdx.x;
  const Slab s = slab_of(n);
  uint64_t base = skip + offs[blockIdx.x];
  uint32_t m[kVec] = {0, 0, 0, 0};
  if (s.lo < s.end) load_masks(mask, n, s.lo, lane, m);
  for (uint64_t t = s.lo; t < s.end; ++t) {
    const uint64_t left = n - t * kSparseTile;
    const uint32_t valid = left < kSparseTile ? (uint32_t)left : kSparseTile;
    uint32_t off[kVec], next[kVec] = {0, 0, 0, 0};
    const uint32_t run = tile_offsets(m, off);
    const uint32_t skew = (uint32_t)base & 15u;
    const uint8_t* src = vals + (base - skew);
    const uint32_t nvec = run ? (skew + run + 15) >> 4 : 0;  // <= 257 aligned vectors of vals: the last one holds the run's last byte
    uint4 w[kVec];
#pragma unroll
    for (int j = 0; j < kVec; ++j)
      if (j * kWave + lane < nvec) w[j] = ld16(src + (j * kWave + lane) * 16);
    if (t + 1 < s.end) load_masks(mask, n, t + 1, lane, next);
#pragma unroll
    for (int j = 0; j < kVec; ++j)
      if (j * kWave + lane < nvec) stage[j * kWave + lane] = w[j];
    if (kTileVecs + lane < nvec) stage[kTileVecs + lane] = ld16(src + (kTileVecs + lane) * 16);
    wave_sync();
    uint4 v[kVec];
#pragma unroll
    for (int j = 0; j < kVec; ++j) v[j] = window16(s32, skew + off[j]);  // at most dword (15 + 4096) / 4 + 4 = 1031 of the 1032
    uint8_t* dst = out + t * kSparseTile;
#pragma unroll
    for (int j = 0; j < kVec; ++j) {
      uint4 x = make_uint4(0, 0, 0, 0);
      uint32_t i = 0;
      for (uint32_t mm = m[j]; mm; mm &= mm - 1) put_byte(x, __builtin_ctz(mm), byte_of(v[j], i++));
      const uint32_t at = (j * kWave + lane) * 16;
      if (at + 16 <= valid) {
        st16(dst + at, x);
      } else if (at < valid) {  // the string's last bytes
        for (uint32_t k = at; k < valid; ++k) dst[k] = (uint8_t)byte_of(x, k - at);
      }
    }
    wave_sync();
    base += run;
#pragma unroll
    for (int j = 0; j < kVec; ++j) m[j] = next[j];
  }
}

__global__ __launch_bounds__(kWave) void k_sparse_merge_move(const uint8_t* __restrict__ mask, const uint8_t* __restrict__ vals, uint64_t n,
                                                             uint8_t* __restrict__ out, const uint64_t* __restrict__ offs,
                                                             const int* __restrict__ status) {
  __shared__ uint4 stage[kStageVecs];
  sparse_merge_move(stage, mask, vals, 0, n, out, offs, status);
}

// ghf_sparse_merge_at: the values are vals[skip .. skip + n_vals).  Nothing in front of
// vals[skip & ~15] and nothing behind the vector that holds the last value is read.  A sibling, not a parameter of the kernel
// above: that one keeps its symbol and its listing.
__global__ __launch_bounds__(kWave) void k_sparse_merge_move_at(const uint8_t* __restrict__ mask, const uint8_t* __restrict__ vals, uint64_t skip,
                                                                uint64_t n, uint8_t* __restrict__ out, const uint64_t* __restrict__ offs,
                                                                const int* __restrict__ status) {
  __shared__ uint4 stage[kStageVecs];
  sparse_merge_move(stage, mask, vals, skip, n, out, offs, status);
}

// ---- the rank table, launch 3: cum[j] = the non-zero bytes in front of element kSparseRankElems * j ------
// Launches 1 and 2 are k_sparse_merge_count and k_sparse_scan.  Every workgroup walks the mask bytes of its slab again, eight
// tiles (one rank block: 4096 mask bytes, four vectors per lane) at a time.  Exactly one of eight consecutive tiles opens a rank
// block; if it lies in the slab this workgroup owns it, whichever slab the rest of the block falls into, and stores its cum
// entry: the slab's offset, the vectors walked so far, and the vectors of this step in front of the tile.  The workgroup with
// the string's last tile also stores cum[blocks] and the header.  Stores nothing behind a latched status.
constexpr uint32_t kRankTiles = kSparseRankElems / kSparseTile;  // 8
constexpr uint32_t kMaskTileVecs = kMaskTileBytes / 16;          // 32
static_assert(kRankTiles * kMaskTileVecs == kTileVecs, "a rank block of mask bytes is one step of the wave");
__global__ __launch_bounds__(kWave) void k_sparse_rank_write(const uint8_t* __restrict__ mask, uint64_t n, const uint64_t* __restrict__ offs,
                                                             uint64_t* __restrict__ table, const int* __restrict__ status) {
  if (__builtin_amdgcn_readfirstlane(*status) != 0) return;
  const uint32_t lane = threadIdx.x;
  const Slab s = slab_of(n);
  if (s.lo >= s.end) return;
  const uint64_t mb = (n + 7) / 8;
  const uint64_t lo = s.lo * kMaskTileBytes, hi = s.end * kMaskTileBytes < mb ? s.end * kMaskTileBytes : mb;  // lo is a multiple of 16
  const uint64_t nv = (hi - lo + 15) / 16;
  uint64_t* const cum = table + kSparseRankHeaderBytes / 8;
  uint64_t running = offs[blockIdx.x];
  for (uint64_t t0 = s.lo; t0 < s.end; t0 += kRankTiles) {
    const uint64_t v0 = (t0 - s.lo) * kMaskTileVecs;
    const uint64_t opens = (t0 + kRankTiles - 1) & ~(uint64_t)(kRankTiles - 1);  // the tile of [t0, t0 + 8) that opens a rank block
    const uint32_t cut = (uint32_t)(opens - t0) * kMaskTileVecs;                 // this step's vectors in front of it
    uint4 x[kVec];
#pragma unroll
    for (int j = 0; j < kVec; ++j) {
      const uint64_t v = v0 + j * kWave + lane;
      x[j] = make_uint4(0, 0, 0, 0);
      if (v < nv) x[j] = ld16(mask + lo + v * 16);
    }
    uint32_t all = 0, front = 0;
#pragma unroll
    for (int j = 0; j < kVec; ++j) {
      const uint64_t v = v0 + j * kWave + lane;
      if (v < nv && hi - lo - v * 16 < 16) x[j] = trim16(x[j], (int)(hi - lo - v * 16));  // behind the last mask byte: not ours
      const uint32_t c = __builtin_popcount(x[j].x) + __builtin_popcount(x[j].y) + __builtin_popcount(x[j].z) + __builtin_popcount(x[j].w);
      all += c;
      front += (uint32_t)(j * kWave) + lane < cut ? c : 0u;
    }
    const uint32_t front_sum = wave_last_u32(wave_incl_scan_u32(front)), all_sum = wave_last_u32(wave_incl_scan_u32(all));
    if (lane == 0 && opens < s.end) cum[opens / kRankTiles] = running + front_sum;
    running += all_sum;
  }
  const uint64_t nt = (n + kSparseTile - 1) / kSparseTile;
  if (s.end == nt) {
    const uint64_t blocks = (n + kSparseRankElems - 1) / kSparseRankElems;
    if (lane == 0) cum[blocks] = running;
    if (lane < kSparseRankHeaderBytes / 8) {
      const uint64_t w = lane == 0   ? kSparseRankMagic
                         : lane == 1 ? (uint64_t)kSparseRankElems << 32 | kSparseRankVersion
                         : lane == 2 ? n
                         : lane == 3 ? running
                         : lane == 4 ? blocks
                                     : 0ull;
      table[lane] = w;
    }
  }
}

// one resident round: kSparseGroups one-wave workgroups, each with a slab of tiles
static uint32_t sparse_grid(uint64_t n) {
  const uint64_t nt = (n + kSparseTile - 1) / kSparseTile;
  return (uint32_t)(nt > kSparseGroups ? kSparseGroups : nt);
}

void launch_sparse_split(const uint8_t* d_in, uint64_t n, uint8_t* d_mask, uint8_t* d_vals, uint64_t vals_cap, uint64_t* d_n_vals,
                         uint64_t* d_counts, uint64_t* d_offs, int* d_status, hipStream_t s) {
  const uint32_t groups = sparse_grid(n);
  const dim3 grid(groups), block(kWave);
  hipLaunchKernelGGL(k_sparse_split_count, grid, block, 0, s, d_in, n, d_mask, d_counts);
  hipLaunchKernelGGL(k_sparse_scan, dim3(1), dim3(kScanThreads), 0, s, d_counts, groups, d_offs, vals_cap, d_n_vals, d_status);
  hipLaunchKernelGGL(k_sparse_split_move, grid, block, 0, s, d_in, n, d_vals, vals_cap, d_offs);
}

void launch_sparse_merge(const uint8_t* d_mask, const uint8_t* d_vals, uint64_t n_vals, uint64_t n, uint8_t* d_out, uint64_t* d_counts,
                         uint64_t* d_offs, int* d_status, hipStream_t s) {
  const uint32_t groups = sparse_grid(n);
  const dim3 grid(groups), block(kWave);
  hipLaunchKernelGGL(k_sparse_merge_count, grid, block, 0, s, d_mask, n, d_counts, d_status);
  hipLaunchKernelGGL(k_sparse_scan, dim3(1), dim3(kScanThreads), 0, s, d_counts, groups, d_offs, n_vals, (uint64_t*)nullptr, d_status);
  hipLaunchKernelGGL(k_sparse_merge_move, grid, block, 0, s, d_mask, d_vals, n, d_out, d_offs, d_status);
}

void launch_sparse_merge_at(const uint8_t* d_mask, const uint8_t* d_vals, uint64_t vals_skip, uint64_t n_vals, uint64_t n, uint8_t* d_out,
                            uint64_t* d_counts, uint64_t* d_offs, int* d_status, hipStream_t s) {
  const uint32_t groups = sparse_grid(n);
  const dim3 grid(groups), block(kWave);
  hipLaunchKernelGGL(k_sparse_merge_count, grid, block, 0, s, d_mask, n, d_counts, d_status);
  hipLaunchKernelGGL(k_sparse_scan, dim3(1), dim3(kScanThreads), 0, s, d_counts, groups, d_offs, n_vals, (uint64_t*)nullptr, d_status);
  hipLaunchKernelGGL(k_sparse_merge_move_at, grid, block, 0, s, d_mask, d_vals, vals_skip, n, d_out, d_offs, d_status);
}

void launch_sparse_rank_pack(const uint8_t* d_mask, uint64_t n, uint8_t* d_table, uint64_t* d_counts, uint64_t* d_offs, int* d_status,
                             hipStream_t s) {
  const uint32_t groups = sparse_grid(n);
  const dim3 grid(groups), block(kWave);
  hipLaunchKernelGGL(k_sparse_merge_count, grid, block, 0, s, d_mask, n, d_counts, d_status);
  // the scan as the split uses it, with no capacity to exceed; the total goes to the spare word behind offs[groups]
  hipLaunchKernelGGL(k_sparse_scan, dim3(1), dim3(kScanThreads), 0, s, d_counts, groups, d_offs, ~0ull, d_offs + kSparseOffWords - 1, d_status);
  hipLaunchKernelGGL(k_sparse_rank_write, grid, block, 0, s, d_mask, n, d_offs, reinterpret_cast<uint64_t*>(d_table), d_status);
}

}  // namespace ghf
