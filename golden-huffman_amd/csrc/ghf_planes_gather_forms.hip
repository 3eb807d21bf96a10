// golden-huffman_amd/csrc/ghf_planes_gather_forms.hip -- many rows of a byte-plane tensor stored in any mix of the three forms,
// against a base tensor where there is one (ghf_decode_planes_gather_forms, include/ghf.h), gfx950 / wave64.
//
// The tensor is stored as ghf_compress_planes_forms stores it: plane p is raw, a standalone .crs2 image with a seek table, or
// SPARSE -- the image of its mask (bit k & 7 of byte k >> 3 says whether byte k is non-zero) in slot p, the image of its
// non-zero bytes in slot E + p, each with a seek table, and a rank table cum[j] = the non-zero bytes in front of element
// 32768 j.  Row r is elements [index[r] * index_stride, + row_elems); one workgroup of 256 threads takes a row and its planes
// in turn, as k_decode_planes_gather does, and raw and dense planes go the way they go there (gather_row).  For a sparse plane
// the mask bytes from the start of the row's rank block to the row's end are decoded with the run walker (ghf_gather_core.h:
// one lane per run of 512 mask bytes), popcounts over the stage give the rank of the row's first element and the number of
// its values, the runs of the values stream that hold them are decoded, and a scan over the row's mask words gives every
// element the number of its value.  Nothing in a table or a stream is trusted, and every verdict of a row, of all planes, is
// reached before its first store: a failed row writes nothing.
#include "ghf_code_rules.h"
#include "ghf_gather_core.h"

namespace ghf {

constexpr uint32_t kFormsStageMax = 48 * 1024;                 // the most dynamic LDS a launch asks for
constexpr uint32_t kRankMaskBytes = kSparseRankElems / 8;      // 4096: the mask bytes of a rank block, one seek block
constexpr uint32_t kRankMaskRuns = kRankMaskBytes / kRunSymbols;  // 8
// a row at the sparse cap covers at most 258 words of the mask; a lane scans two
constexpr uint32_t kFormsMaxWords = (GHF_GATHER_SPARSE_MAX_ROW_ELEMS + 31u) / 32u + 2u;
static_assert(kFormsMaxWords <= 2u * (uint32_t)kBatchThreads, "two mask words per lane, one round");
static_assert(GHF_GATHER_SPARSE_MAX_ROW_ELEMS <= kSparseRankElems, "a row touches at most two rank blocks");

struct GatherFormsLds {  // static; the stage follows as dynamic LDS
  GatherLds g;
  // the launch's arguments, copied here once: read from the kernel's argument segment they are all loaded into scalar
  // registers in front of everything and stay there across the decoder, which has none to spare
  PlanesGatherFormsParams P;
  uint32_t cnt[3];             // set bits in front of the row, of the row's rank block, of the block behind it
  uint32_t wsum[kBatchWaves];  // the scan's wave totals
  uint16_t pre[kFormsMaxWords + 2];  // pre[j]: the row's set bits in front of mask word w0 + j
};

// The parts of the stage, from row_elems alone, so that host and device agree.  A dense plane: the runs of 512 symbols a row
// can touch.  A sparse plane: the runs of 512 mask bytes from the start of a rank block to the end of a row that starts
// anywhere in it, and behind them the runs of its values (no more than row_elems of them, from anywhere in a run).
__host__ __device__ inline uint32_t forms_span_bytes(uint32_t row_elems) {
  return ((uint32_t)kRunSymbols - 1u + row_elems + (uint32_t)kRunSymbols - 1u) / (uint32_t)kRunSymbols * (uint32_t)kRunSymbols;
}
__host__ __device__ inline uint32_t forms_mask_bytes(uint32_t row_elems) {
  const uint32_t bytes = (kSparseRankElems - 1u + row_elems + 7u) / 8u;
  return (bytes + (uint32_t)kRunSymbols - 1u) / (uint32_t)kRunSymbols * (uint32_t)kRunSymbols;
}
static_assert(GHF_GATHER_SPARSE_MAX_ROW_ELEMS / 8 + kRankMaskBytes + 2 * kRunSymbols + (GHF_GATHER_SPARSE_MAX_ROW_ELEMS + 2 * kRunSymbols) <= 16 * 1024,
              "a sparse plane of the longest row stages about 14 KiB");
static_assert(sizeof(GatherFormsLds) + kFormsStageMax <= 64 * 1024, "two workgroups per CU at the longest rows");

// the stage of a launch: every stored plane of a row at once (*once) if that fits, else the largest single plane
inline uint32_t forms_stage_bytes(uint32_t row_elems, uint32_t n_dense, uint32_t n_sparse, uint32_t* once) {
  const uint32_t span = forms_span_bytes(row_elems), sparse = forms_mask_bytes(row_elems) + span;
  const uint32_t all = span * n_dense + sparse * n_sparse;
  *once = all <= kFormsStageMax;
  return all == 0 ? 16u : *once ? all : n_sparse ? sparse : span;
}

// where a row lies among the rank blocks of a sparse plane; the same for every sparse plane of the row
struct RowRanks {
  uint64_t b0;        // the rank block of the row's first element
  uint32_t off;       // that element's place in it
  uint32_t len0;      // the elements of block b0
  uint32_t len1;      // of block b0 + 1 where the row crosses into it, else 0
  uint32_t mend;      // the mask bytes from the start of block b0 to the row's end
  uint32_t nmruns;    // ... in runs of 512
  uint32_t decoded;   // the mask bytes those runs hold: whole runs, cut where the mask ends
  uint32_t pad_from;  // 8 where the row does not touch a last mask byte with pad bits, else the first pad bit
};

// A value that is the same in every lane, kept in a vector register all the same: the row's geometry and its rank entries
// are live across the decoder, whose nested loops need the scalar registers for their lane masks; held in scalar registers
// they are spilled into lanes (the parent kernel sits at 99 of them without this state)
template <class T>
__device__ __forceinline__ T in_lanes(T x) {
  asm volatile("" : "+v"(x));
  return x;
}
// A pointer that went through LDS or through in_lanes has lost what the compiler knew of it; every pointer of the launch is device
// memory, and said so again it is addressed with global_* instructions, not flat_* ones
template <class T>
__device__ __forceinline__ T* in_global(T* p) {
  __attribute__((address_space(1))) T* g = (__attribute__((address_space(1))) T*)p;
  asm volatile("" : "+v"(g));  // (opaque, or the two casts fold away; and a vector register, as in in_lanes)
  return (T*)g;
}
// ... and a verdict back into a scalar, so that the branch on it is one every wave takes whole
__device__ __forceinline__ bool same_in_all(bool x) { return __builtin_amdgcn_readfirstlane((int)x) != 0; }

// the bits of mask word i (elements [32 i, 32 i + 32) of the rank block) that lie below element x
__device__ __forceinline__ uint32_t bits_below(uint32_t i, uint32_t x) {
  const uint32_t lo = 32u * i;
  return x <= lo ? 0u : x >= lo + 32u ? 0xFFFFFFFFu : (1u << (x - lo)) - 1u;
}

// The counts and the scan of a sparse plane whose mask stands in mstage, and the checks they feed.  -> GHF_OK: S.pre holds the
// scan, *v0 the number of the row's first value in the values stream and *nv how many the row has; GHF_E_CORRUPT otherwise.
// Every lane of the workgroup calls it with the same arguments and gets the same verdict; a barrier lies in front of the call
// (the mask is whole) and the caller puts one behind it before S.pre is read.  The checks:
//   where the decoded mask holds a whole rank block -- to the block's end, or the tensor's -- its set bits number the
//   difference of the block's two entries; the row's pad bits are 0; cum[b0] + r0 + nv <= n_vals.
__device__ __forceinline__ int forms_sparse_counts(GatherFormsLds& S, const uint32_t* mstage, const RowRanks& K, uint32_t count, uint64_t c0,
                                                   uint64_t c1, uint64_t c2, uint64_t n_vals, uint64_t* v0, uint32_t* nv_out) {
  // (not a loop invariant of the caller's plane loop: the lane masks of the predicates below would be kept across it)
  const int tid = in_lanes((int)threadIdx.x);
  // the counts: over every decoded word (the run walker leaves zeros behind the mask's last byte, up to a vector)
  {
    uint32_t a = 0, t0 = 0, t1 = 0;
    const uint32_t nwords = (K.decoded + 3u) / 4u;
    for (uint32_t i = tid; i < nwords; i += kBatchThreads) {
      const uint32_t w = mstage[i];
      const uint32_t m0 = bits_below(i, K.len0);
      a += __builtin_popcount(w & bits_below(i, K.off));
      t0 += __builtin_popcount(w & m0);
      t1 += __builtin_popcount(w & ~m0 & bits_below(i, K.len0 + K.len1));
    }
    if (a) atomicAdd(&S.cnt[0], a);
    if (t0) atomicAdd(&S.cnt[1], t0);
    if (t1) atomicAdd(&S.cnt[2], t1);
  }
  // the scan: lane t takes words w0 + 2 t and w0 + 2 t + 1 of the row, cut to the row's own bits
  const uint32_t w0 = K.off / 32u, nw = (K.off + count + 31u) / 32u - w0;  // <= kFormsMaxWords
  uint32_t ca = 0, cb = 0;
  {
    const uint32_t end = K.off + count;
    const uint32_t ja = 2u * tid, jb = ja + 1u;
    if (ja < nw) ca = __builtin_popcount(mstage[w0 + ja] & ~bits_below(w0 + ja, K.off) & bits_below(w0 + ja, end));
    if (jb < nw) cb = __builtin_popcount(mstage[w0 + jb] & ~bits_below(w0 + jb, K.off) & bits_below(w0 + jb, end));
  }
  uint32_t incl = ca + cb;
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const uint32_t up = __shfl_up(incl, d, kWave);
    if ((tid & (kWave - 1)) >= d) incl += up;
  }
  if ((tid & (kWave - 1)) == kWave - 1) S.wsum[tid >> 6] = incl;
  __syncthreads();
  uint32_t front = 0, nv = 0;
#pragma unroll
  for (int w = 0; w < kBatchWaves; ++w) {
    const uint32_t v = S.wsum[w];
    if (w < (tid >> 6)) front += v;
    nv += v;
  }
  const uint32_t excl = front + incl - (ca + cb);
  if (2u * tid < nw) S.pre[2 * tid] = (uint16_t)excl;
  if (2u * tid + 1u < nw) S.pre[2 * tid + 1] = (uint16_t)(excl + ca);
  const uint32_t r0 = S.cnt[0], t0 = S.cnt[1], t1 = S.cnt[2];
  // a rank block the decoded mask holds whole: block b0 ends at mask byte ceil(len0 / 8), the one behind it ceil(len1 / 8) later
  const uint32_t end0 = (K.len0 + 7u) / 8u, end1 = kRankMaskBytes + (K.len1 + 7u) / 8u;
  bool bad = false;
  if (K.decoded >= end0 && (uint64_t)t0 != c1 - c0) bad = true;
  if (K.len1 && K.decoded >= end1 && (uint64_t)t1 != c2 - c1) bad = true;
  if (K.pad_from < 8u && (reinterpret_cast<const uint8_t*>(mstage)[K.mend - 1u] >> K.pad_from) != 0) bad = true;
  if (c0 + r0 + nv > n_vals) bad = true;  // (no overflow: c0 <= n_vals <= n_elems, and the counts are below 2^17)
  *v0 = c0 + r0;
  *nv_out = nv;
  return same_in_all(bad) ? (int)GHF_E_CORRUPT : (int)GHF_OK;
}

// One row.  Every lane of the workgroup calls it with the same arguments and gets the same verdict.  The verdicts come in this
// order, all before the first store: the row lies inside the tensor (GHF_E_INVAL); every stored plane agrees with its streams
// and tables (GHF_E_CORRUPT).  Step s < E judges plane s -- and keeps it, where the launch's stage holds every plane of a row
// at once (P.once); step E + p lets plane p leave, and where the stage holds one plane decodes it again in front of its stores.
// A plane has up to two stored streams, taken in turn by ONE loop so that the decoder is laid out once: the plane itself or
// its mask, and the values of a sparse plane.  For a sparse plane, in order: the rank entries of the row's blocks are ordered,
// not above n_vals, and no step exceeds the elements of its block; every covered block and run of the mask stream agrees with
// the stream (gather_decode_runs); the counts (forms_sparse_counts); every covered run of the values stream.  Where the first
// pass kept the plane only the counts and the scan are made again.  A raw plane is read where it lies.  The way out of the
// stage is StorePlane's: one byte store per symbol at stride E; with a base the byte of the base element is read beside it and
// XORed in.  Only bytes [0, row_elems * E) of the output row are written.
template <int E>
__device__ __forceinline__ int gather_forms_row(GatherFormsLds& S, uint32_t* stage0, const PlanesGatherFormsParams& P, uint32_t raw,
                                                uint32_t sparse, uint64_t idx, uint8_t* out) {
  const int tid = threadIdx.x;
  const uint64_t n = P.n_elems;
  const uint32_t count = P.row_elems;
  if (__umul64hi(idx, P.index_stride) != 0) return GHF_E_INVAL;  // the product overflows 64 bits
  const uint64_t first = in_lanes(idx * P.index_stride);
  if (same_in_all(first > n || (uint64_t)count > n - first)) return GHF_E_INVAL;
  const uint32_t skip = (uint32_t)(first % kRunSymbols);
  const uint32_t span_words = in_lanes(forms_span_bytes(count) / 4u), mask_words = in_lanes(forms_mask_bytes(count) / 4u);
  out = in_global(in_lanes(out));
  const bool once = P.once != 0;
  RowRanks K = {};
  if (sparse) {  // count <= GHF_GATHER_SPARSE_MAX_ROW_ELEMS, and first < n
    K.b0 = first / kSparseRankElems;
    K.off = (uint32_t)(first % kSparseRankElems);
    const uint64_t left = n - K.b0 * kSparseRankElems;  // the elements from the start of block b0 on
    K.len0 = left < kSparseRankElems ? (uint32_t)left : kSparseRankElems;
    const bool crosses = K.off + count > kSparseRankElems;  // then block b0 is whole and block b0 + 1 exists
    K.len1 = !crosses ? 0u : left - kSparseRankElems < kSparseRankElems ? (uint32_t)(left - kSparseRankElems) : kSparseRankElems;
    K.mend = (K.off + count + 7u) / 8u;
    K.nmruns = (K.mend + kRunSymbols - 1) / kRunSymbols;
    const uint64_t mask_left = (left + 7) / 8;  // the mask bytes from the start of block b0 on: >= mend
    K.decoded = (uint64_t)K.nmruns * kRunSymbols < mask_left ? K.nmruns * kRunSymbols : (uint32_t)mask_left;
    K.pad_from = (first + count + 7) / 8 == (n + 7) / 8 && (n & 7u) ? (uint32_t)(n & 7u) : 8u;
    K.b0 = in_lanes(K.b0), K.off = in_lanes(K.off), K.len0 = in_lanes(K.len0), K.len1 = in_lanes(K.len1), K.mend = in_lanes(K.mend);
    K.nmruns = in_lanes(K.nmruns), K.decoded = in_lanes(K.decoded), K.pad_from = in_lanes(K.pad_from);
  }

  if (tid == 0) S.g.err = 0;  // (the barriers of batch_code_tables lie between this and the runs)
  uint32_t part = 0;
#pragma unroll 1
  for (uint32_t s = 0; s < 2 * E; ++s) {
    const uint32_t p = s % E;
    const int tl = in_lanes(tid);  // the lane, opaque per plane: no predicate on it is kept in a lane mask across the loop
    const bool leaves = s >= E, is_raw = (raw >> p & 1u) != 0, is_sparse = (sparse >> p & 1u) != 0;  // (the same in every lane)
    if (s == E) {
      __syncthreads();
      if (S.g.err) return GHF_E_CORRUPT;
      part = 0;
    }
    uint32_t* const stage = stage0 + (once ? part : 0u);
    const bool decode = !is_raw && !(leaves && once);
    uint64_t c0 = 0, c1 = 0, c2 = 0, v0 = 0;
    uint32_t nv = 0;
    if (is_sparse) {
      const uint64_t* const cum = in_global(P.cum[p]) + K.b0;  // b0 + 1 <= rank blocks, and b0 + 2 <= rank blocks where the row crosses
      c0 = cum[0], c1 = cum[1], c2 = K.len1 ? cum[2] : c1;
      if (same_in_all(c0 > c1 || c1 > c2 || c2 > P.n_vals[p] || c1 - c0 > (uint64_t)K.len0 || c2 - c1 > (uint64_t)K.len1)) return GHF_E_CORRUPT;
    }
#pragma unroll 1
    for (uint32_t sub = 0; sub < (is_sparse ? 2u : 1u); ++sub) {  // the plane or its mask; a sparse plane's values
      if (is_sparse) {
        __syncthreads();  // the lanes are done with the stage, the counts and the scan of the stream before this one
        if (S.g.err) return GHF_E_CORRUPT;  // (sub 1: what stands in the stage is not the mask)
        if (sub == 0) {
          if (tl < 3) S.cnt[tl] = 0;
        } else {
          if (forms_sparse_counts(S, stage, K, count, c0, c1, c2, P.n_vals[p], &v0, &nv)) return GHF_E_CORRUPT;
        }
      }
      if (decode && (sub == 0 || same_in_all(nv != 0))) {
        const uint32_t j = sub ? E + p : p;
        const uint64_t symbols = sub ? P.n_vals[p] : is_sparse ? (n + 7) / 8 : n;
        const uint64_t r0 = sub ? v0 / kRunSymbols : is_sparse ? K.b0 * kRankMaskRuns : first / kRunSymbols;
        const uint32_t nr = sub ? ((uint32_t)(v0 % kRunSymbols) + nv + kRunSymbols - 1) / kRunSymbols
                                : is_sparse ? K.nmruns : (skip + count + kRunSymbols - 1) / kRunSymbols;
        if (leaves) __syncthreads();  // the stores of the plane before this one have read the stage
        int lb, long_from, max_len;
        batch_code_tables(S.g.t, in_global(P.codes) + j, tl, lb, long_from, max_len);
        gather_decode_runs(S.g, stage + (sub ? mask_words : 0u), in_global(P.streams[j]), P.stream_bytes[j], in_global(P.records[j]), blocks_for(symbols), symbols,
                           r0, nr, lb, long_from, max_len);
        if (leaves) __syncthreads();
      }
    }
    if (is_sparse) {
      __syncthreads();  // the scan and the values are whole
      if (S.g.err) return GHF_E_CORRUPT;
    }
    if (leaves) {
      uint8_t* const dst = out + p;
      const uint8_t* const bsrc = P.base ? in_global(P.base) + first * E + p : nullptr;
      if (is_sparse) {
        const uint32_t w0 = K.off / 32u;
        const uint8_t* const vals = reinterpret_cast<const uint8_t*>(stage + mask_words) + (uint32_t)(v0 % kRunSymbols);
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
        for (uint32_t k = tl; k < count; k += kBatchThreads) {
          const uint32_t b = K.off + k, wi = b / 32u;
          uint32_t w = stage[wi];
          uint32_t v = 0;
          if (w >> (b & 31u) & 1u) {
            w &= (1u << (b & 31u)) - 1u;
            if (wi == w0) w &= ~((1u << (K.off & 31u)) - 1u);
            v = vals[(uint32_t)S.pre[wi - w0] + __builtin_popcount(w)];
          }
          if (bsrc) v ^= bsrc[(size_t)k * E];
          dst[(size_t)k * E] = (uint8_t)v;
        }
      } else {
        // a raw plane is the plane itself: n bytes, held against n_elems on the host
        const uint8_t* const raw_src = in_global(P.streams[p]) + first;
        const uint8_t* const sb = reinterpret_cast<const uint8_t*>(stage) + skip;
        // (a loop per source: one pointer for both would be neither LDS nor device memory, and every load a flat one)
        if (is_raw) {
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
          for (uint32_t k = tl; k < count; k += kBatchThreads) dst[(size_t)k * E] = raw_src[k] ^ (bsrc ? bsrc[(size_t)k * E] : 0);
        } else {
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
          for (uint32_t k = tl; k < count; k += kBatchThreads) dst[(size_t)k * E] = sb[k] ^ (bsrc ? bsrc[(size_t)k * E] : 0);
        }
      }
    }
    if (!is_raw) part += is_sparse ? mask_words + span_words : span_words;
  }
  return GHF_OK;
}

// One workgroup per row, rows beyond 65536 in the grid's second dimension, as in k_decode_planes_gather.  The codes of every
// stored stream that has one -- a dense plane's, a mask's, the values' of a sparse plane that has any -- are vetted in front of
// everything (GHF_E_FORMAT on every row; nothing is written).  The masks are kernel arguments: the same in every wave.
constexpr uint32_t kFormsGridX = 65536;

template <int E>
__global__ __launch_bounds__(kBatchThreads) void k_decode_planes_gather_forms(PlanesGatherFormsParams P, uint32_t raw, uint32_t sparse) {
  __shared__ GatherFormsLds S;
  extern __shared__ __attribute__((aligned(16))) uint32_t forms_stage[];  // P.stage_bytes of them
  const int tid = threadIdx.x;
  const uint64_t r = (uint64_t)blockIdx.y * gridDim.x + blockIdx.x;
  if (r >= P.n_rows) return;
  static_assert(sizeof(PlanesGatherFormsParams) % 4 == 0, "copied by words");
  for (uint32_t i = tid; i < sizeof(PlanesGatherFormsParams) / 4; i += kBatchThreads)
    reinterpret_cast<uint32_t*>(&S.P)[i] = reinterpret_cast<const uint32_t*>(&P)[i];
  __syncthreads();
  const PlanesGatherFormsParams& Q = S.P;
  bool codes_ok = true;
#pragma unroll 1
  for (uint32_t j = 0; j < 2 * E; ++j) {
    const uint32_t p = j % E;
    const bool coded = j < E ? !(raw >> p & 1u) : (sparse >> p & 1u) && Q.n_vals[p] != 0;
    if (coded) codes_ok &= batch_code_ok(S.g.vet, in_global(Q.codes) + j, tid);
  }
  const int status = codes_ok ? gather_forms_row<E>(S, forms_stage, Q, raw, sparse, in_global(Q.index)[r], in_global(Q.out) + r * Q.out_stride) : (int)GHF_E_FORMAT;
  if (tid == 0) in_global(Q.row_status)[r] = status;
}

void launch_decode_planes_gather_forms(const PlanesGatherFormsParams& params, uint32_t elem_bytes, uint32_t raw_planes, uint32_t sparse_planes,
                                       hipStream_t s) {
  if (params.n_rows == 0) return;
  PlanesGatherFormsParams p = params;
  const uint32_t n_sparse = (uint32_t)__builtin_popcount(sparse_planes);
  p.stage_bytes = forms_stage_bytes(p.row_elems, elem_bytes - (uint32_t)__builtin_popcount(raw_planes) - n_sparse, n_sparse, &p.once);
  const uint32_t gx = p.n_rows < kFormsGridX ? p.n_rows : kFormsGridX;
  const dim3 grid(gx, (uint32_t)(((uint64_t)p.n_rows + gx - 1) / gx)), block(kBatchThreads);
  with_elem_bytes(elem_bytes, [&](auto e) {
    hipLaunchKernelGGL(k_decode_planes_gather_forms<decltype(e)::value>, grid, block, p.stage_bytes, s, p, raw_planes, sparse_planes);
  });
}

}  // namespace ghf
