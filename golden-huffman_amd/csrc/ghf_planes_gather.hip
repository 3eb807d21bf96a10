// golden-huffman_amd/csrc/ghf_planes_gather.hip -- many rows of a byte-plane compressed tensor in one launch
// (ghf_decode_planes_gather, include/ghf.h), gfx950 / wave64.
//
// The tensor is stored as ghf_compress_planes_forms stores it without sparse planes: plane p is a standalone .crs2 image
// with a seek table, or raw.  Row r is elements [index[r] * index_stride, + row_elems); one
// workgroup of 256 threads takes a row and its planes in turn.  For a dense plane the small decoder of the batch family
// (ghf_batch_core.h) is filled from the plane's code and ONE LANE TAKES EVERY RUN of 512 symbols that the row touches: it
// forms the run's start bit from its block's record, decodes the run once into the LDS stage and must land on the recorded
// end.  A raw plane is read where it lies.  Nothing in a table or a stream is trusted, and every verdict of a row is
// reached before its first store: a failed row writes nothing.
#include "ghf_code_rules.h"
#include "ghf_gather_core.h"

namespace ghf {

// the runs of 512 symbols a row of r elements can touch: ceil(r / 512) + 1
constexpr uint32_t kGatherMaxRuns = GHF_GATHER_MAX_ROW_ELEMS / kRunSymbols + 1;  // 65
static_assert(kGatherMaxRuns <= (uint32_t)kBatchThreads, "one lane per run, one round");
// The stage holds the decoded runs of one plane of the row -- or of ALL dense planes of a row short enough, which are then
// decoded once (gather_row below).  It is the launch's dynamic LDS, sized by the host from row_elems (gather_stage_bytes):
// 33 280 bytes for one plane at the row cap, at most 48 KiB, and for short rows so little that the 9 KiB of tables decide
// how many workgroups a CU holds.  The walk of a run is a chain of dependent loads, so resident rows are what hides it.
constexpr uint32_t kGatherStageMax = 48 * 1024;
static_assert(kGatherStageMax >= kGatherMaxRuns * kRunSymbols, "the stage holds one plane of the longest row");

// (GatherLds, the static part, stands with the run walker in ghf_gather_core.h)
static_assert(sizeof(GatherLds) + kGatherStageMax <= 64 * 1024, "two workgroups per CU at the longest rows");

// the stage of a launch: every dense plane of the longest run span a row of row_elems can have, if that fits; else one plane
inline uint32_t gather_stage_bytes(uint32_t row_elems, uint32_t n_dense) {
  const uint32_t span = ((uint32_t)kRunSymbols - 1u + row_elems + (uint32_t)kRunSymbols - 1u) / (uint32_t)kRunSymbols * (uint32_t)kRunSymbols;
  const uint32_t all = span * n_dense;
  return all == 0 ? 16u : all <= kGatherStageMax ? all : span;
}

// (gather_decode_runs, the run walker: ghf_gather_core.h, shared with ghf_planes_gather_forms.hip)

// One row.  Every lane of the workgroup calls it with the same arguments and gets the same verdict.  The verdicts come in
// this order, all before the first store: the row lies inside the tensor (GHF_E_INVAL); every covered block and run of
// every dense plane agrees with its stream (GHF_E_CORRUPT).  Where the runs of all dense planes fit the stage together
// they are decoded ONCE, each plane into a part of its own; at longer rows the first pass only judges and each plane is
// decoded again in front of its stores.  The way out of the stage is StorePlane's: one byte store per symbol at stride E,
// so that a wave's stores fall on consecutive elements; only bytes [0, row_elems * E) of the output row are written, at
// any alignment.  (The store loops are kept from being interleaved four deep: the trip masks that brings stay alive
// across the plane loop and push scalar registers out into lanes.)
template <int E>
__device__ __forceinline__ int gather_row(GatherLds& S, uint32_t* stage0, const PlanesGatherParams& P, uint32_t raw, uint64_t idx,
                                          uint8_t* out) {
  const int tid = threadIdx.x;
  const uint64_t n = P.n_elems;
  const uint32_t count = P.row_elems;
  if (__umul64hi(idx, P.index_stride) != 0) return GHF_E_INVAL;  // the product overflows 64 bits
  const uint64_t first = idx * P.index_stride;
  if (first > n || (uint64_t)count > n - first) return GHF_E_INVAL;
  const uint64_t run0 = first / kRunSymbols;
  const uint32_t skip = (uint32_t)(first % kRunSymbols);
  const uint32_t nruns = (skip + count + kRunSymbols - 1) / kRunSymbols;  // <= kGatherMaxRuns
  const uint32_t part_words = nruns * (kRunSymbols / 4);
  const uint32_t n_dense = (uint32_t)__builtin_popcount(~raw & ((1u << E) - 1u));
  const bool once = n_dense * part_words * 4u <= P.stage_bytes;  // (else stage_bytes holds one plane: nruns * 512 at the most)

  if (tid == 0) S.err = 0;  // (the barriers of batch_code_tables lie between this and the runs)
  // step s < E: plane s is judged (and kept, under `once`); step E + p: plane p leaves.  One loop, so that the decoder is
  // laid out once
  uint32_t part = 0;
#pragma unroll 1
  for (uint32_t s = 0; s < 2 * E; ++s) {
    const uint32_t p = s % E;
    const bool leaves = s >= E, is_raw = (raw >> p & 1u) != 0;  // (the same in every lane, as is all control flow here)
    if (s == E) {
      __syncthreads();
      if (n_dense && S.err) return GHF_E_CORRUPT;
      part = 0;
    }
    uint32_t* const stage = stage0 + (once ? part : 0u);
    if (!is_raw && !(leaves && once)) {
      if (leaves) __syncthreads();  // the stores of the plane before this one have read the stage
      int lb, long_from, max_len;
      batch_code_tables(S.t, P.codes + p, tid, lb, long_from, max_len);
      gather_decode_runs(S, stage, P.streams[p], P.stream_bytes[p], P.records[p], P.n_blocks, n, run0, nruns, lb, long_from, max_len);
      if (leaves) __syncthreads();
    }
    if (leaves) {
      // a raw plane is the plane itself: n bytes, held against n_elems on the host
      uint8_t* const dst = out + p;
      if (is_raw) {
        const uint8_t* const src = P.streams[p] + first;
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
        for (uint32_t k = tid; k < count; k += kBatchThreads) dst[(size_t)k * E] = src[k];
      } else {
        const uint8_t* const sb = reinterpret_cast<const uint8_t*>(stage) + skip;
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
        for (uint32_t k = tid; k < count; k += kBatchThreads) dst[(size_t)k * E] = sb[k];
      }
    }
    if (!is_raw) part += part_words;
  }
  return GHF_OK;
}

// One workgroup per row: row = blockIdx.y * gridDim.x + blockIdx.x (rows beyond 65536 go to the grid's second dimension, and
// the workgroups behind row n_rows - 1 of the last line leave at once).  A workgroup that looped over rows would keep
// the row's lane masks alive across the loop: more scalar registers than there are.  The codes of the dense planes are
// vetted in front of everything (GHF_E_FORMAT on every row; nothing is written).  `raw` is a kernel argument: the same in
// every wave.  Failures are the row's own: nothing is latched anywhere.
constexpr uint32_t kGatherGridX = 65536;

template <int E>
__global__ __launch_bounds__(kBatchThreads) void k_decode_planes_gather(PlanesGatherParams P, uint32_t raw) {
  __shared__ GatherLds S;
  extern __shared__ __attribute__((aligned(16))) uint32_t gather_stage[];  // P.stage_bytes of them
  const int tid = threadIdx.x;
  const uint64_t r = (uint64_t)blockIdx.y * gridDim.x + blockIdx.x;
  if (r >= P.n_rows) return;
  bool codes_ok = true;
#pragma unroll 1
  for (uint32_t p = 0; p < E; ++p)
    if (!(raw >> p & 1u)) codes_ok &= batch_code_ok(S.vet, P.codes + p, tid);
  const int status = codes_ok ? gather_row<E>(S, gather_stage, P, raw, P.index[r], P.out + r * P.out_stride) : (int)GHF_E_FORMAT;
  if (tid == 0) P.row_status[r] = status;
}

void launch_decode_planes_gather(const PlanesGatherParams& params, uint32_t elem_bytes, uint32_t raw_planes, hipStream_t s) {
  if (params.n_rows == 0) return;
  PlanesGatherParams p = params;
  p.stage_bytes = gather_stage_bytes(p.row_elems, elem_bytes - (uint32_t)__builtin_popcount(raw_planes));
  const uint32_t gx = p.n_rows < kGatherGridX ? p.n_rows : kGatherGridX;
  const dim3 grid(gx, (uint32_t)(((uint64_t)p.n_rows + gx - 1) / gx)), block(kBatchThreads);
  with_elem_bytes(elem_bytes, [&](auto e) { hipLaunchKernelGGL(k_decode_planes_gather<decltype(e)::value>, grid, block, p.stage_bytes, s, p, raw_planes); });
}

}  // namespace ghf
