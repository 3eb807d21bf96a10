// golden-huffman_amd/csrc/ghf_planes.hip -- byte planes of typed elements.
// k_planes_split<E>: d_in[0 .. n_elems * E) -> E planes, byte b of element k at planes + b * plane_stride + k.
// k_planes_merge<E>: the inverse.  E = 2, 4, 8.  Both move N bytes in and N bytes out and nothing else; they are judged as
// streaming kernels against k_stream_copy (ghf_kernels.hip) and keep its access shape: every global access of the main loop
// is one 16-byte vector per lane with consecutive lanes on consecutive vectors -- on the interleaved side and on every
// plane --, max(E, 4) loads are in flight per lane before the first use, the non-temporal hint on both sides, and one
// resident round of workgroups that each stream through a contiguous slab of tiles.
//
// One wave = one workgroup = one tile at a time.  A tile is 64 * max(E, 4) vectors of the interleaved side, cut into ROWS
// of E vectors = 16 elements.  The row is the unit of the transposition: a lane that holds a row's E vectors turns them
// into one 16-byte vector of each plane with v_perm_b32 alone (byte 4x4 transposes).  Rows reach their lanes through the
// wave's LDS tile: the interleaved side is loaded (stored) with lane l on vector 64 j + l, the row side reads (writes) the
// E consecutive vectors of row l.  A row is padded by one vector, (E + 1) * 16 bytes: the ds_read_b128 / ds_write_b128 of
// the row side, 16 lanes (8 lanes) at that stride, then fall on distinct banks for every E (12, 20, 36 dwords: 4 * odd).
// The LDS carries 2 N bytes at 16 bytes per lane and instruction; no barrier is needed, the tile is private to its wave.
//
// The tile is written twice, split_body and merge_body; the nine kernels -- split, merge and the skewed merge of a range
// (section 17), each plain, against a base tensor (_delta, section 19) and with one address per plane (_to / _from, section
// 23) -- are one call of a body each, which takes base, skew and the shape of the plane addresses as compile-time switches.
#include "ghf_device.h"

namespace ghf {

namespace {

template <int E>
struct PlanesGeom {
  static constexpr int kVec = E < 4 ? 4 : E;           // 16-byte loads in flight per lane
  static constexpr int kRows = kWave * kVec / E;       // rows of 16 elements per tile
  static constexpr int kRowsPerLane = kVec / E;        // 2 (E = 2) or 1
  static constexpr int kRowVec = E + 1;                // a row in LDS, in vectors: padded by one
  static constexpr uint32_t kTile = planes_tile_elems(E);
  static_assert(kTile == (uint32_t)kRows * 16, "the tile the host counts with");
  static_assert(kRows * kRowVec * 16 <= (int)kPlanesLdsBytes, "the LDS budget of DESIGN.md section 14");
};

__device__ __forceinline__ uint32_t perm(uint32_t hi, uint32_t lo, uint32_t sel) { return __builtin_amdgcn_perm(hi, lo, sel); }

// 4x4 byte transpose: o[b] byte k = byte b of i_k.  Its own inverse.
__device__ __forceinline__ void transpose4(uint32_t i0, uint32_t i1, uint32_t i2, uint32_t i3, uint32_t& o0, uint32_t& o1,
                                           uint32_t& o2, uint32_t& o3) {
  const uint32_t lo01 = perm(i1, i0, 0x05010400u), hi01 = perm(i1, i0, 0x07030602u);  // {i0.b0 i1.b0 i0.b1 i1.b1}, {.. b2 .. b3}
  const uint32_t lo23 = perm(i3, i2, 0x05010400u), hi23 = perm(i3, i2, 0x07030602u);
  o0 = perm(lo23, lo01, 0x05040100u);
  o1 = perm(lo23, lo01, 0x07060302u);
  o2 = perm(hi23, hi01, 0x05040100u);
  o3 = perm(hi23, hi01, 0x07060302u);
}

__device__ __forceinline__ uint32_t& word(uint4& v, int q) { return q == 0 ? v.x : q == 1 ? v.y : q == 2 ? v.z : v.w; }
__device__ __forceinline__ uint32_t word(const uint4& v, int q) { return q == 0 ? v.x : q == 1 ? v.y : q == 2 ? v.z : v.w; }

// a row's E vectors (16 elements) -> one vector of each plane.  Dword d of the row is word d % 4 of r[d / 4].
template <int E>
__device__ __forceinline__ void row_to_planes(const uint4 (&r)[E], uint4 (&p)[E]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {  // elements 4 q .. 4 q + 3 -> dword q of every plane
    if constexpr (E == 2) {
      const uint32_t a = word(r[q / 2], 2 * q % 4), b = word(r[q / 2], 2 * q % 4 + 1);
      word(p[0], q) = perm(b, a, 0x06040200u);
      word(p[1], q) = perm(b, a, 0x07050301u);
    } else if constexpr (E == 4) {
      transpose4(r[q].x, r[q].y, r[q].z, r[q].w, word(p[0], q), word(p[1], q), word(p[2], q), word(p[3], q));
    } else {  // an element is two dwords: the even ones hold planes 0..3, the odd ones planes 4..7
      transpose4(r[2 * q].x, r[2 * q].z, r[2 * q + 1].x, r[2 * q + 1].z, word(p[0], q), word(p[1], q), word(p[2], q), word(p[3], q));
      transpose4(r[2 * q].y, r[2 * q].w, r[2 * q + 1].y, r[2 * q + 1].w, word(p[4], q), word(p[5], q), word(p[6], q), word(p[7], q));
    }
  }
}

template <int E>
__device__ __forceinline__ void planes_to_row(const uint4 (&p)[E], uint4 (&r)[E]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if constexpr (E == 2) {
      const uint32_t a = word(p[0], q), b = word(p[1], q);
      word(r[q / 2], 2 * q % 4) = perm(b, a, 0x05010400u);
      word(r[q / 2], 2 * q % 4 + 1) = perm(b, a, 0x07030602u);
    } else if constexpr (E == 4) {
      transpose4(word(p[0], q), word(p[1], q), word(p[2], q), word(p[3], q), r[q].x, r[q].y, r[q].z, r[q].w);
    } else {
      transpose4(word(p[0], q), word(p[1], q), word(p[2], q), word(p[3], q), r[2 * q].x, r[2 * q].z, r[2 * q + 1].x, r[2 * q + 1].z);
      transpose4(word(p[4], q), word(p[5], q), word(p[6], q), word(p[7], q), r[2 * q].y, r[2 * q].w, r[2 * q + 1].y, r[2 * q + 1].w);
    }
  }
}

// the hint of k_stream_copy<true>, K1 and K7 on both sides: every byte is touched once.  (`make nt_ab` builds the -DGHF_PLANES_NT=0
// variant for the A/B of DESIGN.md section 14, tools/planes_nt_ab.py.)
#ifndef GHF_PLANES_NT
#define GHF_PLANES_NT 1
#endif
__device__ __forceinline__ uint4 ld16(const uint4* p) { return GHF_PLANES_NT ? load_stream(p) : *p; }
__device__ __forceinline__ void st16(uint4* p, const uint4& v) {
  if (GHF_PLANES_NT) store_stream(p, v);
  else *p = v;
}

// the slab of whole tiles this workgroup streams through (as k_stream_copy cuts its vectors), and the ragged end: the
// elements behind the last whole tile, one per lane, spread over the grid (launch_planes makes the grid wide enough)
struct Slab {
  uint64_t lo, end, tail;
};
__device__ __forceinline__ Slab slab_of(uint64_t n_elems, uint32_t tile) {
  const uint64_t nt = n_elems / tile, per = (nt + gridDim.x - 1) / gridDim.x;
  const uint64_t lo = (uint64_t)blockIdx.x * per;
  return {lo, lo + per < nt ? lo + per : nt, nt * tile + (uint64_t)blockIdx.x * kWave + threadIdx.x};
}

// bytes [skew, skew + 16) of the 32 bytes lo || hi, skew = 1 .. 15 and wave-uniform: the dword part of the skew picks five of
// the eight dwords (two rounds of uniform v_cndmask_b32), the byte part funnels neighbours with v_alignbyte_b32
__device__ __forceinline__ uint4 funnel16(const uint4& lo, const uint4& hi, uint32_t skew) {
  const bool by1 = skew & 4u, by2 = skew & 8u;
  const uint32_t y0 = by1 ? lo.y : lo.x, y1 = by1 ? lo.z : lo.y, y2 = by1 ? lo.w : lo.z, y3 = by1 ? hi.x : lo.w;
  const uint32_t y4 = by1 ? hi.y : hi.x, y5 = by1 ? hi.z : hi.y, y6 = by1 ? hi.w : hi.z;
  const uint32_t x0 = by2 ? y2 : y0, x1 = by2 ? y3 : y1, x2 = by2 ? y4 : y2, x3 = by2 ? y5 : y3, x4 = by2 ? y6 : y4;
  const uint32_t b = skew & 3u;
  return make_uint4(__builtin_amdgcn_alignbyte(x1, x0, b), __builtin_amdgcn_alignbyte(x2, x1, b),
                    __builtin_amdgcn_alignbyte(x3, x2, b), __builtin_amdgcn_alignbyte(x4, x3, b));
}

__device__ __forceinline__ uint4 xor16(const uint4& a, const uint4& b) { return make_uint4(a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w); }

// ----------------------------------------------------------------------------------------------------------------------
// WHERE THE PLANES ARE, in two shapes.  Both give vec(b, t, r, lane), the 16-byte vector of plane b for row r * kWave + lane
// of tile t, and byte(b, k), byte k of plane b.  B is uint8_t on the split's side, const uint8_t on the merge's.
// ----------------------------------------------------------------------------------------------------------------------
template <class B>
using vec_of = std::conditional_t<std::is_const<B>::value, const uint4, uint4>;

// one pointer and one stride: plane b starts at p + b * stride
template <int E, class B>
struct StridedPlanes {
  static constexpr bool kPerPlane = false;
  B* p;
  uint64_t stride;
  __device__ __forceinline__ vec_of<B>* vec(int b, uint64_t t, int r, uint32_t lane) const {
    return reinterpret_cast<vec_of<B>*>(p + b * stride) + t * PlanesGeom<E>::kRows + r * kWave + lane;
  }
  __device__ __forceinline__ B& byte(int b, uint64_t k) const { return p[b * stride + k]; }
};

// ONE ADDRESS PER PLANE: a plane stored raw lives in the caller's image, the others in the context's
// workspace, and one pointer and one stride cannot name both.  The E addresses travel by value in the kernel arguments: they
// are wave-uniform, every index into them is a constant once the loops are unrolled, and they stay in SGPRs.
template <int E, class B>
struct PlaneAddrs {
  static constexpr bool kPerPlane = true;
  B* p[E];
  __device__ __forceinline__ vec_of<B>* vec(int b, uint64_t t, int r, uint32_t lane) const {
    return reinterpret_cast<vec_of<B>*>(p[b] + (t * PlanesGeom<E>::kRows + r * kWave) * 16) + lane;
  }
  __device__ __forceinline__ B& byte(int b, uint64_t k) const { return p[b][k]; }
};

}  // namespace

// the parameter types of the pointer kernels (their names are part of the kernels' symbols)
template <int E>
struct PlaneDsts : PlaneAddrs<E, uint8_t> {};
template <int E>
struct PlaneSrcs : PlaneAddrs<E, const uint8_t> {};

namespace {

// ----------------------------------------------------------------------------------------------------------------------
// THE TWO BODIES.  Every kernel of this unit is one call of one of them; the `if constexpr` switches leave each kernel the
// instruction stream it would have written out by hand (DESIGN.md section 19 has the rule the listings are held to).
//
// kDelta: the planes are those of in ^ base, the merge gives back planes ^ base.  `base` holds the
// bytes of the interleaved side -- of a range: the range's own elements, base[0 .. n_elems * E), with no skew -- and is read
// with the interleaved side's access shape: lane l on vector 64 j + l of the tile, 16 bytes per lane, the non-temporal
// hint.  Its max(E, 4) loads are issued together with the tile's other loads, before the first LDS instruction, and the XOR
// is applied to registers: on the way into the LDS tile in the split, on the way out of it in the merge (whose base load so
// never waits behind the transposition).  Nothing outside base[0 .. n_elems * E) is read; without kDelta `base` is not
// looked at.
// ----------------------------------------------------------------------------------------------------------------------
template <int E, bool kDelta, class P>
__device__ __forceinline__ void split_body(const uint8_t* in, const uint8_t* base, uint64_t n_elems, const P& dst) {
  using G = PlanesGeom<E>;
  __shared__ uint4 tile[G::kRows * G::kRowVec];
  const uint32_t lane = threadIdx.x;
  const Slab s = slab_of(n_elems, G::kTile);
  for (uint64_t t = s.lo; t < s.end; ++t) {
    const uint4* src = reinterpret_cast<const uint4*>(in) + t * (kWave * G::kVec);
    uint4 x[G::kVec], d[G::kVec];
#pragma unroll
    for (int j = 0; j < G::kVec; ++j) x[j] = ld16(src + j * kWave + lane);
    if constexpr (kDelta) {
      const uint4* bsrc = reinterpret_cast<const uint4*>(base) + t * (kWave * G::kVec);
#pragma unroll
      for (int j = 0; j < G::kVec; ++j) d[j] = ld16(bsrc + j * kWave + lane);
    }
#pragma unroll
    for (int j = 0; j < G::kVec; ++j) {
      const uint32_t v = j * kWave + lane;
      if constexpr (kDelta) tile[(v / E) * G::kRowVec + v % E] = xor16(x[j], d[j]);
      else tile[(v / E) * G::kRowVec + v % E] = x[j];
    }
    wave_sync();
#pragma unroll
    for (int r = 0; r < G::kRowsPerLane; ++r) {
      const uint32_t row = r * kWave + lane;
      uint4 y[E], p[E];
#pragma unroll
      for (int j = 0; j < E; ++j) y[j] = tile[row * G::kRowVec + j];
      row_to_planes<E>(y, p);
#pragma unroll
      for (int b = 0; b < E; ++b) st16(dst.vec(b, t, r, lane), p[b]);
    }
    wave_sync();
  }
  for (uint64_t k = s.tail; k < n_elems; k += (uint64_t)gridDim.x * kWave) {  // the ragged end: byte by byte
#pragma unroll
    for (int b = 0; b < E; ++b) {
      if constexpr (kDelta) dst.byte(b, k) = in[k * E + b] ^ base[k * E + b];
      else dst.byte(b, k) = in[k * E + b];
    }
  }
}

// status (may be null): the context's latched status word; a launch that finds it non-zero stores nothing (one read per
// workgroup, the convention of k_decode) -- the planes of a failed decode are not merged.
//
// kSkew: the run of n_elems elements starts `skew` = 1 .. 15 bytes into a 16-byte vector of EVERY
// plane; the addresses in `src` are 16-byte aligned (the caller has taken the skew off them; skew == 0 is the kernel
// without kSkew, which does not look at `skew`).  The same tiles, slabs, LDS rows and stores; on the plane side a lane loads
// the two ALIGNED vectors that hold its 16 bytes and funnels them.  The second vector of the last row of the last whole
// tile ends at or before the vector that holds element skew + n_elems - 1 (skew > 0), so nothing outside
// [0, (skew + n_elems + 15) & ~15) of a plane is read.
//
// kDelta: `out` and `base` may be the SAME pointer ("XOR the delta into the base"), which is why the shells give neither a
// __restrict__: a lane reads the base vector (the base bytes of the ragged end) that it overwrites itself, and every load
// of a tile's base is issued before the tile's first store.
template <int E, bool kDelta, bool kSkew, class P>
__device__ __forceinline__ void merge_body(const P& src, uint32_t skew, const uint8_t* base, uint64_t n_elems, uint8_t* out,
                                           const int* status) {
  using G = PlanesGeom<E>;
  __shared__ uint4 tile[G::kRows * G::kRowVec];
  if (status && __builtin_amdgcn_readfirstlane(*status) != 0) return;
  const uint32_t lane = threadIdx.x;
  if constexpr (kSkew) skew = __builtin_amdgcn_readfirstlane(skew);
  const Slab s = slab_of(n_elems, G::kTile);
  for (uint64_t t = s.lo; t < s.end; ++t) {
    uint4 p[G::kRowsPerLane][E], hi[G::kRowsPerLane][E], d[G::kVec];
#pragma unroll
    for (int r = 0; r < G::kRowsPerLane; ++r)
#pragma unroll
      for (int b = 0; b < E; ++b) {
        const uint4* v = src.vec(b, t, r, lane);
        p[r][b] = ld16(v);
        if constexpr (kSkew) hi[r][b] = ld16(v + 1);
      }
    if constexpr (kDelta) {
      const uint4* bsrc = reinterpret_cast<const uint4*>(base) + t * (kWave * G::kVec);
#pragma unroll
      for (int j = 0; j < G::kVec; ++j) d[j] = ld16(bsrc + j * kWave + lane);
      // k_planes_merge_from<E, true> alone: every load of the tile is issued before the first use.  Left
      // to itself the scheduler sinks two of the sixteen loads of E = 8 below the transposition, and orders those of E = 2, 4
      // otherwise; every other kernel has all its loads in front unaided, or pays for the barrier with a wave (section 23)
      if constexpr (P::kPerPlane && !kSkew) __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int r = 0; r < G::kRowsPerLane; ++r) {
      const uint32_t row = r * kWave + lane;
      uint4 y[E];
      if constexpr (kSkew) {
#pragma unroll
        for (int b = 0; b < E; ++b) p[r][b] = funnel16(p[r][b], hi[r][b], skew);
      }
      planes_to_row<E>(p[r], y);
#pragma unroll
      for (int j = 0; j < E; ++j) tile[row * G::kRowVec + j] = y[j];
    }
    wave_sync();
    uint4* dst = reinterpret_cast<uint4*>(out) + t * (kWave * G::kVec);
#pragma unroll
    for (int j = 0; j < G::kVec; ++j) {
      const uint32_t v = j * kWave + lane;
      if constexpr (kDelta) st16(dst + j * kWave + lane, xor16(tile[(v / E) * G::kRowVec + v % E], d[j]));
      else st16(dst + j * kWave + lane, tile[(v / E) * G::kRowVec + v % E]);
    }
    wave_sync();
  }
  for (uint64_t k = s.tail; k < n_elems; k += (uint64_t)gridDim.x * kWave) {
#pragma unroll
    for (int b = 0; b < E; ++b) {
      if constexpr (kDelta) out[k * E + b] = src.byte(b, kSkew ? skew + k : k) ^ base[k * E + b];
      else out[k * E + b] = src.byte(b, kSkew ? skew + k : k);
    }
  }
}

}  // namespace

// ---- the nine kernels: k_planes_split / _merge / _merge_range, plain, _delta (against a base) and _to / _from (one address
// per plane).  n_elems > 0; every pointer, every plane address and plane_stride 16-byte aligned -------------------------------
template <int E>
__global__ __launch_bounds__(kWave) void k_planes_split(const uint8_t* __restrict__ in, uint64_t n_elems, uint8_t* __restrict__ planes,
                                                        uint64_t plane_stride) {
  split_body<E, false>(in, nullptr, n_elems, StridedPlanes<E, uint8_t>{planes, plane_stride});
}
template <int E>
__global__ __launch_bounds__(kWave) void k_planes_split_delta(const uint8_t* __restrict__ in, const uint8_t* __restrict__ base,
                                                              uint64_t n_elems, uint8_t* __restrict__ planes, uint64_t plane_stride) {
  split_body<E, true>(in, base, n_elems, StridedPlanes<E, uint8_t>{planes, plane_stride});
}
template <int E, bool kDelta>
__global__ __launch_bounds__(kWave) void k_planes_split_to(const uint8_t* __restrict__ in, const uint8_t* __restrict__ base,
                                                           uint64_t n_elems, PlaneDsts<E> dst) {
  split_body<E, kDelta>(in, base, n_elems, dst);
}

template <int E>
__global__ __launch_bounds__(kWave) void k_planes_merge(const uint8_t* __restrict__ planes, uint64_t plane_stride, uint64_t n_elems,
                                                        uint8_t* __restrict__ out, const int* __restrict__ status) {
  merge_body<E, false, false>(StridedPlanes<E, const uint8_t>{planes, plane_stride}, 0, nullptr, n_elems, out, status);
}
template <int E>
__global__ __launch_bounds__(kWave) void k_planes_merge_range(const uint8_t* __restrict__ planes, uint64_t plane_stride, uint32_t skew,
                                                              uint64_t n_elems, uint8_t* __restrict__ out,
                                                              const int* __restrict__ status) {
  merge_body<E, false, true>(StridedPlanes<E, const uint8_t>{planes, plane_stride}, skew, nullptr, n_elems, out, status);
}
template <int E>
__global__ __launch_bounds__(kWave) void k_planes_merge_delta(const uint8_t* __restrict__ planes, uint64_t plane_stride,
                                                              const uint8_t* base, uint64_t n_elems, uint8_t* out,
                                                              const int* __restrict__ status) {
  merge_body<E, true, false>(StridedPlanes<E, const uint8_t>{planes, plane_stride}, 0, base, n_elems, out, status);
}
template <int E>
__global__ __launch_bounds__(kWave) void k_planes_merge_range_delta(const uint8_t* __restrict__ planes, uint64_t plane_stride,
                                                                    uint32_t skew, const uint8_t* base, uint64_t n_elems, uint8_t* out,
                                                                    const int* __restrict__ status) {
  merge_body<E, true, true>(StridedPlanes<E, const uint8_t>{planes, plane_stride}, skew, base, n_elems, out, status);
}
template <int E, bool kDelta>
__global__ __launch_bounds__(kWave) void k_planes_merge_from(PlaneSrcs<E> src, const uint8_t* base, uint64_t n_elems, uint8_t* out,
                                                             const int* __restrict__ status) {
  merge_body<E, kDelta, false>(src, 0, base, n_elems, out, status);
}
template <int E, bool kDelta>
__global__ __launch_bounds__(kWave) void k_planes_merge_range_from(PlaneSrcs<E> src, uint32_t skew, const uint8_t* base, uint64_t n_elems,
                                                                   uint8_t* out, const int* __restrict__ status) {
  merge_body<E, kDelta, true>(src, skew, base, n_elems, out, status);
}

// ---- launchers -----------------------------------------------------------------------------------------------------------
// one resident round: kPlanesGroups one-wave workgroups, each with a slab of whole tiles; at least one lane per element of
// the ragged end
static uint32_t planes_grid(uint64_t n_elems, uint32_t elem_bytes) {
  const uint32_t tile = planes_tile_elems(elem_bytes);
  const uint64_t nt = n_elems / tile, tail_waves = (n_elems % tile + kWave - 1) / kWave;
  const uint64_t g = nt > tail_waves ? nt : tail_waves;
  return (uint32_t)(g > kPlanesGroups ? kPlanesGroups : g);
}

// d_base == nullptr: the plain kernel; else the planes of d_in ^ d_base, on the same grid
void launch_planes_split(const uint8_t* d_in, const uint8_t* d_base, uint64_t n_elems, uint32_t elem_bytes, uint8_t* d_planes,
                         uint64_t plane_stride, hipStream_t s) {
  const dim3 grid(planes_grid(n_elems, elem_bytes)), block(kWave);
  with_elem_bytes(elem_bytes, [&](auto e) {
    constexpr int E = decltype(e)::value;
    if (d_base) hipLaunchKernelGGL(k_planes_split_delta<E>, grid, block, 0, s, d_in, d_base, n_elems, d_planes, plane_stride);
    else hipLaunchKernelGGL(k_planes_split<E>, grid, block, 0, s, d_in, n_elems, d_planes, plane_stride);
  });
}

// d_base == nullptr: the plain kernel; else d_out = merge(planes) ^ d_base, d_base == d_out allowed
void launch_planes_merge(const uint8_t* d_planes, uint64_t plane_stride, const uint8_t* d_base, uint64_t n_elems, uint32_t elem_bytes,
                         uint8_t* d_out, const int* d_status, hipStream_t s) {
  const dim3 grid(planes_grid(n_elems, elem_bytes)), block(kWave);
  with_elem_bytes(elem_bytes, [&](auto e) {
    constexpr int E = decltype(e)::value;
    if (d_base) hipLaunchKernelGGL(k_planes_merge_delta<E>, grid, block, 0, s, d_planes, plane_stride, d_base, n_elems, d_out, d_status);
    else hipLaunchKernelGGL(k_planes_merge<E>, grid, block, 0, s, d_planes, plane_stride, n_elems, d_out, d_status);
  });
}

// elements [first, first + count) of the planes; a range that starts on a vector is k_planes_merge on the shifted planes.
// d_base (may be null) holds base elements [first, first + count) at d_base[0 .. count * elem_bytes): it carries no skew,
// only the planes do
void launch_planes_merge_range(const uint8_t* d_planes, uint64_t plane_stride, const uint8_t* d_base, uint64_t first, uint64_t count,
                               uint32_t elem_bytes, uint8_t* d_out, const int* d_status, hipStream_t s) {
  const uint32_t skew = (uint32_t)(first & 15u);
  const uint8_t* from = d_planes + (first - skew);
  if (skew == 0) return launch_planes_merge(from, plane_stride, d_base, count, elem_bytes, d_out, d_status, s);
  const dim3 grid(planes_grid(count, elem_bytes)), block(kWave);
  with_elem_bytes(elem_bytes, [&](auto e) {
    constexpr int E = decltype(e)::value;
    if (d_base)
      hipLaunchKernelGGL(k_planes_merge_range_delta<E>, grid, block, 0, s, from, plane_stride, skew, d_base, count, d_out, d_status);
    else hipLaunchKernelGGL(k_planes_merge_range<E>, grid, block, 0, s, from, plane_stride, skew, count, d_out, d_status);
  });
}

void launch_planes_split_to(const uint8_t* d_in, const uint8_t* d_base, uint64_t n_elems, uint32_t elem_bytes, uint8_t* const* h_dst,
                            hipStream_t s) {
  const dim3 grid(planes_grid(n_elems, elem_bytes)), block(kWave);
  with_elem_bytes(elem_bytes, [&](auto e) {
    constexpr int E = decltype(e)::value;
    PlaneDsts<E> dst;
    for (int b = 0; b < E; ++b) dst.p[b] = h_dst[b];
    if (d_base) hipLaunchKernelGGL((k_planes_split_to<E, true>), grid, block, 0, s, d_in, d_base, n_elems, dst);
    else hipLaunchKernelGGL((k_planes_split_to<E, false>), grid, block, 0, s, d_in, d_base, n_elems, dst);
  });
}

// h_src[b] is plane b's byte of the first element; all have the same address mod 16 (the caller has seen to it)
void launch_planes_merge_from(const uint8_t* const* h_src, const uint8_t* d_base, uint64_t n_elems, uint32_t elem_bytes, uint8_t* d_out,
                              const int* d_status, hipStream_t s) {
  const dim3 grid(planes_grid(n_elems, elem_bytes)), block(kWave);
  const uint32_t skew = (uint32_t)(reinterpret_cast<uintptr_t>(h_src[0]) & 15u);
  with_elem_bytes(elem_bytes, [&](auto e) {
    constexpr int E = decltype(e)::value;
    PlaneSrcs<E> src;
    for (int b = 0; b < E; ++b) src.p[b] = h_src[b] - skew;
    if (skew == 0) {
      if (d_base) hipLaunchKernelGGL((k_planes_merge_from<E, true>), grid, block, 0, s, src, d_base, n_elems, d_out, d_status);
      else hipLaunchKernelGGL((k_planes_merge_from<E, false>), grid, block, 0, s, src, d_base, n_elems, d_out, d_status);
    } else {
      if (d_base) hipLaunchKernelGGL((k_planes_merge_range_from<E, true>), grid, block, 0, s, src, skew, d_base, n_elems, d_out, d_status);
      else hipLaunchKernelGGL((k_planes_merge_range_from<E, false>), grid, block, 0, s, src, skew, d_base, n_elems, d_out, d_status);
    }
  });
}

}  // namespace ghf
