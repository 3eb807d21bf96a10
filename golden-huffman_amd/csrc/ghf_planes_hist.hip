// golden-huffman_amd/csrc/ghf_planes_hist.hip -- the staged form of the byte-plane path for ONE large typed buffer
// (ghf_histogram_planes, ghf_planes_image_bytes, ghf_compress_planes_coded, include/ghf.h).
//
// k_histogram_planes<E>: the E plane histograms of d_in[0 .. n_elems * E) in one pass over the interleaved buffer, E = 2, 4, 8.
// The planes are never materialised: E divides 16, so byte k of an aligned 16-byte vector belongs to plane k % E.
//
// LDS layout: K1's (ghf_kernels.hip) -- bins[256][32] u32, 32 KiB for every E, ds_add_u32 whose bank is the COLUMN of the
// counter.  K1 gives every lane of a 32-lane LDS group a column of its own (replica = lane % 32), which makes the add
// conflict-free for any byte distribution.  Here the 32 columns are E planes x R = 32 / E replicas, column = plane * R + rep,
// and a lane of the group is (q, rep) = (lane % 32 / R, lane % R).  If every lane counted byte k of its vector in step k,
// all lanes of an instruction would stand on one plane, R columns, and the E lanes that share a replica would collide
// whenever their bytes differ (and serialise on one address where they agree: the skewed high plane).  So the lanes ROTATE
// through the bytes: in step s a lane counts byte (s + q) % 8 of a pair of dwords, plane (s + q) % E.  The E lanes that
// share a replica then stand on E different planes, the 32 lanes of a group on 32 different columns = banks, in every step
// and for every input; lanes l and l + 32 are served in different LDS cycles, as in K1.  The byte is picked by v_perm_b32
// with a per-lane selector (selector byte 0x0c reads as zero), so a count costs what it costs in K1: one extract, one
// v_lshl_or_b32, one ds_add_u32.  The 8 selectors and 8 column offsets of a lane are loop-invariant registers.
//
// One resident round of kPlanesHistGroups persistent workgroups (4 on each CU: 4 x 32 KiB of LDS, K1's occupancy) strides
// over tiles of 256 threads x 4 vectors = 16 KiB; a tile's four non-temporal loads are in flight while the tile before
// it is counted.  Every kPlanesHistFlushTiles tiles, and at its end, a workgroup sums its columns per plane into u64
// registers (thread t owns bin t; running sums and differences mod 2^32 as in K1, so nothing is re-zeroed): a u32 counter
// gains at most the bytes its workgroup counted since the last flush, kPlanesHistFlushTiles * 16 KiB + one ragged tile.  The
// whole vectors behind the last tile and the < 16 bytes behind them are counted by the workgroup next in turn, with guarded
// loads and bytewise; nothing beyond d_in[n_elems * E) is read.  No per-chunk histograms are kept.  At its end a workgroup
// adds its E x 256 sums into one of 32 replicas in global memory (blockIdx % 32: a word sees 32 adds instead of 1024);
// k_histogram_planes_finish, the next launch, sums the replicas, leaves them zeroed for the next call, and writes the
// caller's E x 257 counts (slot 256 = 1, GHF_HIST_COVER_ALL per plane).
#include "ghf_code_rules.h"
#include "ghf_device.h"

namespace ghf {

static_assert(kPlanesHistCols == 32 && kPlanesHistThreads == 256, "column = bank; thread t owns bin t");

template <int E>
struct PlanesHistLane {
  uint32_t sel[8];   // v_perm_b32 selector of step s: byte (s + q) % 8 of {hi, lo}, zero-extended
  uint32_t col4[8];  // byte offset of the lane's column in step s: 4 * (plane * R + rep)
  __device__ __forceinline__ explicit PlanesHistLane(uint32_t tid) {
    constexpr uint32_t R = kPlanesHistCols / E;
    const uint32_t q = (tid & 31u) / R, rep = tid % R;
#pragma unroll
    for (uint32_t s = 0; s < 8; ++s) {
      const uint32_t j = (s + q) & 7u;
      sel[s] = 0x0c0c0c00u | j;
      col4[s] = 4u * ((j % E) * R + rep);
    }
  }
};

// bytes 0 .. 7 of {hi, lo}, each into its plane
template <int E>
__device__ __forceinline__ void planes_hist_pair(uint8_t* lds, const PlanesHistLane<E>& L, uint32_t lo, uint32_t hi) {
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    const uint32_t b = __builtin_amdgcn_perm(hi, lo, L.sel[s]);
    atomicAdd(reinterpret_cast<uint32_t*>(lds + ((b << 7) | L.col4[s])), 1u);
  }
}
template <int E>
__device__ __forceinline__ void planes_hist_vec(uint8_t* lds, const PlanesHistLane<E>& L, const uint4& v) {
  planes_hist_pair<E>(lds, L, v.x, v.y);  // E divides 8: byte k of either pair belongs to plane k % E
  planes_hist_pair<E>(lds, L, v.z, v.w);
}

template <int E>
__global__ __launch_bounds__(kPlanesHistThreads, 4) void k_histogram_planes(const uint8_t* __restrict__ in, uint64_t n_bytes,
                                                                         unsigned long long* __restrict__ acc /* [32][E][256] */) {
  constexpr uint32_t R = kPlanesHistCols / E;
  __shared__ __attribute__((aligned(16))) uint32_t lh[256 * kPlanesHistCols];
  uint8_t* const lds = reinterpret_cast<uint8_t*>(lh);
  const uint32_t tid = threadIdx.x;
  const PlanesHistLane<E> L(tid);
  const uint64_t nvec = n_bytes >> 4, ntiles = nvec / kPlanesHistTileVecs;
  const uint4* const src = reinterpret_cast<const uint4*>(in);
  auto load_tile = [&](uint64_t t, uint4 (&x)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = load_stream(src + t * kPlanesHistTileVecs + j * kPlanesHistThreads + tid);
  };
  uint64_t t = blockIdx.x;
  uint4 cur[4] = {}, nxt[4];
  if (t < ntiles) load_tile(t, cur);  // the first round trip to HBM hides behind the clearing of the counters
  for (uint32_t i = tid; i < 256 * kPlanesHistCols; i += kPlanesHistThreads) lh[i] = 0;
  __syncthreads();

  // Thread t owns bin t and sums its 32 columns in E groups of R.  Group g of thread t is plane (g + t / R) % E, and inside a
  // group the thread starts at column t % R: the 32 lanes of an LDS group then read 32 different columns = banks in every
  // step.  prev[] / total[] are indexed by the group, which is static; the plane is only needed for the address of the
  // final add.  The counters keep running; what a group gained is the difference to its sum at the flush before (mod 2^32).
  uint32_t prev[E];
  unsigned long long total[E];
#pragma unroll
  for (int g = 0; g < E; ++g) {
    prev[g] = 0;
    total[g] = 0;
  }
  const uint32_t q_t = tid / R, r_t = tid % R;
  auto flush = [&]() {
    __syncthreads();
#pragma unroll
    for (uint32_t g = 0; g < E; ++g) {
      const uint32_t base = (tid << 5) | (((g + q_t) % E) * R);
      uint32_t s = 0;
#pragma unroll
      for (uint32_t r = 0; r < R; ++r) s += lh[base | ((r + r_t) % R)];
      total[g] += s - prev[g];
      prev[g] = s;
    }
    __syncthreads();
  };

  uint32_t since = 0;  // tiles since the last flush; the same in every lane
  // counts tile t out of `a` while the tile after it is on its way into `b`
  auto step = [&](uint4 (&a)[4], uint4 (&b)[4]) {
    const uint64_t tn = t + gridDim.x;
    load_tile(tn < ntiles ? tn : t, b);  // behind the last tile: a redundant, harmless load, so that the wait counts are the same on every path
#pragma unroll
    for (int j = 0; j < 4; ++j) planes_hist_vec<E>(lds, L, a[j]);
    if (++since == kPlanesHistFlushTiles) {
      flush();
      since = 0;
    }
    t = tn;
  };
  while (t < ntiles) {  // the two buffers swap roles without a register copy
    step(cur, nxt);
    if (t >= ntiles) break;
    step(nxt, cur);
  }
  // the ragged end belongs to the workgroup that would take tile `ntiles`: whole vectors, then single bytes
  if (ntiles % gridDim.x == blockIdx.x) {
    for (uint64_t v = ntiles * kPlanesHistTileVecs + tid; v < nvec; v += kPlanesHistThreads) planes_hist_vec<E>(lds, L, src[v]);
    const uint64_t k = (nvec << 4) + tid;  // a multiple of 16 plus tid: plane tid % E
    if (k < n_bytes) atomicAdd(&lh[((uint32_t)in[k] << 5) | ((tid % E) * R)], 1u);
  }
  flush();
  unsigned long long* const mine = acc + (uint64_t)(blockIdx.x & 31u) * (E * 256);
#pragma unroll
  for (uint32_t g = 0; g < E; ++g)
    if (total[g]) atomicAdd(&mine[((g + q_t) % E) * 256 + tid], total[g]);
}

// k_histogram_planes of in ^ base: the same counters, bank rotation, flush rule, grid and ragged end.
// A tile is four vectors of `in` AND the four vectors of `base` at the same offsets, eight non-temporal loads that are in
// flight while the tile before it is counted.  A step XORs the arrived tile in registers -- its base registers are dead
// from then on and receive the next tile's base --, issues the next tile's eight loads and then counts: three buffers of
// four vectors are live, not four, which is what keeps the kernel at its parent's 128 registers and four workgroups on a
// CU.  Nothing outside in[0 .. n_bytes) and base[0 .. n_bytes) is read.  The body stands beside its parent's and shares
// only the lane helpers, so that the parent's instruction stream stays what it was.
template <int E>
__global__ __launch_bounds__(kPlanesHistThreads, 4) void k_histogram_planes_delta(const uint8_t* __restrict__ in,
                                                                               const uint8_t* __restrict__ base, uint64_t n_bytes,
                                                                               unsigned long long* __restrict__ acc /* [32][E][256] */) {
  constexpr uint32_t R = kPlanesHistCols / E;
  __shared__ __attribute__((aligned(16))) uint32_t lh[256 * kPlanesHistCols];
  uint8_t* const lds = reinterpret_cast<uint8_t*>(lh);
  const uint32_t tid = threadIdx.x;
  const PlanesHistLane<E> L(tid);
  const uint64_t nvec = n_bytes >> 4, ntiles = nvec / kPlanesHistTileVecs;
  const uint4* const src = reinterpret_cast<const uint4*>(in);
  const uint4* const bsrc = reinterpret_cast<const uint4*>(base);
  auto load_tile = [&](uint64_t t, uint4 (&x)[4], uint4 (&d)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = load_stream(src + t * kPlanesHistTileVecs + j * kPlanesHistThreads + tid);
#pragma unroll
    for (int j = 0; j < 4; ++j) d[j] = load_stream(bsrc + t * kPlanesHistTileVecs + j * kPlanesHistThreads + tid);
  };
  uint64_t t = blockIdx.x;
  uint4 cur[4] = {}, nxt[4], d[4] = {};
  if (t < ntiles) load_tile(t, cur, d);  // the first round trip to HBM hides behind the clearing of the counters
  for (uint32_t i = tid; i < 256 * kPlanesHistCols; i += kPlanesHistThreads) lh[i] = 0;
  __syncthreads();

  // thread t owns bin t: the sums of k_histogram_planes.  A group's u32 sum at the flush before is the low half of its
  // total (both start at 0 and gain the same differences mod 2^32), so it is not kept a second time: E registers that the
  // third buffer needs
  unsigned long long total[E];
#pragma unroll
  for (int g = 0; g < E; ++g) total[g] = 0;
  const uint32_t q_t = tid / R, r_t = tid % R;
  auto flush = [&]() {
    __syncthreads();
#pragma unroll
    for (uint32_t g = 0; g < E; ++g) {
      const uint32_t col = (tid << 5) | (((g + q_t) % E) * R);
      uint32_t s = 0;
#pragma unroll
      for (uint32_t r = 0; r < R; ++r) s += lh[col | ((r + r_t) % R)];
      total[g] += (uint32_t)(s - (uint32_t)total[g]);
    }
    __syncthreads();
  };

  uint32_t since = 0;  // tiles since the last flush; the same in every lane
  // counts tile t out of a ^ d while the tile after it is on its way into (b, d)
  auto step = [&](uint4 (&a)[4], uint4 (&b)[4]) {
    const uint64_t tn = t + gridDim.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] = make_uint4(a[j].x ^ d[j].x, a[j].y ^ d[j].y, a[j].z ^ d[j].z, a[j].w ^ d[j].w);
    load_tile(tn < ntiles ? tn : t, b, d);  // behind the last tile: a redundant, harmless load (see k_histogram_planes)
#pragma unroll
    for (int j = 0; j < 4; ++j) planes_hist_vec<E>(lds, L, a[j]);
    if (++since == kPlanesHistFlushTiles) {
      flush();
      since = 0;
    }
    t = tn;
  };
  while (t < ntiles) {  // the two input buffers swap roles without a register copy
    step(cur, nxt);
    if (t >= ntiles) break;
    step(nxt, cur);
  }
  // the ragged end belongs to the workgroup that would take tile `ntiles`: whole vectors, then single bytes
  if (ntiles % gridDim.x == blockIdx.x) {
    for (uint64_t v = ntiles * kPlanesHistTileVecs + tid; v < nvec; v += kPlanesHistThreads) {
      const uint4 x = src[v], y = bsrc[v];
      planes_hist_vec<E>(lds, L, make_uint4(x.x ^ y.x, x.y ^ y.y, x.z ^ y.z, x.w ^ y.w));
    }
    const uint64_t k = (nvec << 4) + tid;  // a multiple of 16 plus tid: plane tid % E
    if (k < n_bytes) atomicAdd(&lh[((uint32_t)(uint8_t)(in[k] ^ base[k]) << 5) | ((tid % E) * R)], 1u);
  }
  flush();
  unsigned long long* const mine = acc + (uint64_t)(blockIdx.x & 31u) * (E * 256);
#pragma unroll
  for (uint32_t g = 0; g < E; ++g)
    if (total[g]) atomicAdd(&mine[((g + q_t) % E) * 256 + tid], total[g]);
}

// behind k_histogram_planes on the same stream, one workgroup per plane: sums the 32 replicas and zeroes them again, then
// the end mark counts once (include/encoder.h:123-129); cover: no count stays 0
__global__ __launch_bounds__(256) void k_histogram_planes_finish(unsigned long long* __restrict__ acc, uint32_t elem_bytes,
                                                                 uint64_t* __restrict__ hists, uint32_t cover) {
  const uint32_t tid = threadIdx.x, p = blockIdx.x;
  unsigned long long sum = 0;
#pragma unroll 8
  for (uint32_t r = 0; r < 32; ++r) {
    unsigned long long* const w = acc + ((uint64_t)r * elem_bytes + p) * 256 + tid;
    sum += *w;
    *w = 0;
  }
  uint64_t* const hist = hists + (size_t)p * GHF_NSYM;
  hist[tid] = cover && sum == 0 ? 1 : sum;
  if (tid == 0) hist[256] = 1;
}

// ----------------------------------------------------------------------------------------------------------------------
// One plane's code against one plane's counts, by a workgroup of 256: is the code a complete prefix code (ghf_code_rules.h
// section 2: code_share_ok plus the Kraft sum), has every counted byte a code, and how many body bits do the counts make
// under it (the end mark once, whatever slot 256 says).  Every lane returns the same answer.
// ----------------------------------------------------------------------------------------------------------------------
struct PlaneCodeLds {
  unsigned long long kraft, bits;
  int bad, nocode;
};
struct PlaneCodeVerdict {
  bool complete, covered;
  uint64_t bits;
  int max_len;
};
__device__ __forceinline__ PlaneCodeVerdict plane_code_verdict(PlaneCodeLds& S, const uint64_t* __restrict__ hist,
                                                               const ghf_code* __restrict__ code, int tid) {
  if (tid == 0) {
    S.kraft = 0;
    S.bits = 0;
    S.bad = 0;
    S.nocode = 0;
  }
  __syncthreads();
  const int max_len = code->max_len, min_len = code->min_len;
  const bool bounds = len_bounds_ok(min_len, max_len);  // (the same in every lane)
  if (bounds) {
    unsigned long long k = 0;
    if (!code_share_ok(code, min_len, max_len, tid, 256, &k)) atomicOr(&S.bad, 1);
    if (k) atomicAdd(&S.kraft, k);
    const uint32_t len = code->length[tid];
    const unsigned long long cnt = hist[tid];
    if (cnt && len == 0) atomicOr(&S.nocode, 1);
    unsigned long long b = cnt * len;
    if (tid == 0) {
      const uint32_t end_len = code->length[GHF_NSYM - 1];
      if (end_len == 0) atomicOr(&S.nocode, 1);
      b += end_len;
    }
    if (b) atomicAdd(&S.bits, b);
  }
  __syncthreads();
  PlaneCodeVerdict v;
  v.complete = bounds && S.bad == 0 && S.kraft == (1ull << 32);
  v.covered = S.nocode == 0;
  v.bits = S.bits;
  v.max_len = max_len;
  __syncthreads();  // S may be reused
  return v;
}

// one workgroup per plane: bytes[p] <- the size of the image any compress call writes for counts hists[p] under codes[p];
// 0 when the code is not complete or leaves a counted byte without a code
__global__ __launch_bounds__(256) void k_planes_image_bytes(const uint64_t* __restrict__ hists, const ghf_code* __restrict__ codes,
                                                            uint64_t* __restrict__ bytes) {
  __shared__ PlaneCodeLds S;
  const uint32_t p = blockIdx.x;
  const PlaneCodeVerdict v = plane_code_verdict(S, hists + (size_t)p * GHF_NSYM, codes + p, threadIdx.x);
  if (threadIdx.x == 0) bytes[p] = v.complete && v.covered ? header_bytes_for((uint64_t)v.max_len) + ((v.bits + 7) >> 3) : 0;
}

// one workgroup takes the planes in turn: a code that is not complete latches GHF_E_FORMAT, else a counted byte without a
// code latches GHF_E_NOCODE (the first plane with a complaint, and of its complaints the format, decides)
__global__ __launch_bounds__(256) void k_planes_vet_codes(const uint64_t* __restrict__ hists, const ghf_code* __restrict__ codes,
                                                          uint32_t elem_bytes, int* __restrict__ status) {
  __shared__ PlaneCodeLds S;
  for (uint32_t p = 0; p < elem_bytes; ++p) {
    const PlaneCodeVerdict v = plane_code_verdict(S, hists + (size_t)p * GHF_NSYM, codes + p, threadIdx.x);
    if (v.complete && v.covered) continue;
    if (threadIdx.x == 0) latch_status(status, v.complete ? GHF_E_NOCODE : GHF_E_FORMAT);
    return;
  }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------
// one resident round, or as many workgroups as there are tiles
static uint32_t planes_hist_grid(uint64_t n_bytes) {
  const uint64_t nvec = n_bytes >> 4, ntiles = nvec / kPlanesHistTileVecs;
  const uint64_t g = ntiles + ((n_bytes - ntiles * kPlanesHistTileVecs * 16) != 0);  // the ragged end wants a workgroup too
  return (uint32_t)(g > kPlanesHistGroups ? kPlanesHistGroups : g);
}
// -> the first launch error.  An error of the counting launch means that nothing was queued: the replicas are still zero
// d_base == nullptr: the plain count; else the count of d_in ^ d_base (the same grid, the same finish)
hipError_t launch_histogram_planes(const uint8_t* d_in, const uint8_t* d_base, uint64_t n_elems, uint32_t elem_bytes, uint32_t flags,
                                   uint64_t* d_acc, uint64_t* d_hists, hipStream_t s) {
  const uint64_t n_bytes = n_elems * elem_bytes;
  const dim3 grid(planes_hist_grid(n_bytes)), block(kPlanesHistThreads);
  unsigned long long* const acc = reinterpret_cast<unsigned long long*>(d_acc);
  with_elem_bytes(elem_bytes, [&](auto e) {
    constexpr int E = decltype(e)::value;
    if (d_base) hipLaunchKernelGGL(k_histogram_planes_delta<E>, grid, block, 0, s, d_in, d_base, n_bytes, acc);
    else hipLaunchKernelGGL(k_histogram_planes<E>, grid, block, 0, s, d_in, n_bytes, acc);
  });
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_histogram_planes_finish, dim3(elem_bytes), dim3(256), 0, s, acc, elem_bytes, d_hists,
                     (uint32_t)((flags & GHF_HIST_COVER_ALL) != 0));
  return hipGetLastError();
}

void launch_planes_image_bytes(const uint64_t* d_hists, const ghf_code* d_codes, uint32_t elem_bytes, uint64_t* d_bytes, hipStream_t s) {
  hipLaunchKernelGGL(k_planes_image_bytes, dim3(elem_bytes), dim3(256), 0, s, d_hists, d_codes, d_bytes);
}

void launch_planes_vet_codes(const uint64_t* d_hists, const ghf_code* d_codes, uint32_t elem_bytes, int* d_status, hipStream_t s) {
  hipLaunchKernelGGL(k_planes_vet_codes, dim3(1), dim3(256), 0, s, d_hists, d_codes, elem_bytes, d_status);
}

}  // namespace ghf
