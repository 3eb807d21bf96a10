// golden-huffman_amd/csrc/ghf_tensor.hip -- the container of one typed tensor (GHFTENS1): k_tensor_pack
// lays the stored streams of ghf_compress_planes_forms behind the host-known part of the container and writes the head,
// k_tensor_open vets the .crs2 headers and the table headers of a container that came from anywhere and fills its codes.
#include "ghf_code_rules.h"
#include "ghf_device.h"

namespace ghf {

namespace {

// a vector with the bytes at and behind `rem` (1 .. 15) cleared: the last vector of a stream
__device__ __forceinline__ uint4 keep_bytes(uint4 v, uint32_t rem) {
  const uint32_t full = rem >> 2, part = (1u << (8 * (rem & 3u))) - 1u;  // part == 0 when the cut falls between two words
  v.x = full > 0 ? v.x : v.x & part;  // rem >= 1: word 0 is whole or cut
  v.y = full > 1 ? v.y : full == 1 ? v.y & part : 0u;
  v.z = full > 2 ? v.z : full == 2 ? v.z & part : 0u;
  v.w = full == 3 ? v.w & part : 0u;
  return v;
}

// what one lane of a k_tensor_pack workgroup decides for all of it
enum PackVerdict : uint32_t { kPackGo = 0, kPackLatched, kPackCap, kPackEmpty };

__device__ __forceinline__ uint32_t ld_be32(const uint8_t* p) { return bswap32(*reinterpret_cast<const uint32_t*>(p)); }
__device__ __forceinline__ uint32_t ld_le32(const uint8_t* p) { return *reinterpret_cast<const uint32_t*>(p); }
__device__ __forceinline__ uint64_t ld_le64(const uint8_t* p) { return *reinterpret_cast<const uint64_t*>(p); }

}  // namespace

// ------------------------------------------------------------------------------------------------
// k_tensor_pack.  ONE launch.  Every workgroup reads the up to 16 device sizes and forms the same exclusive scan of the
// padded sizes: no workgroup waits for another.  One lane forms the verdict -- a latched status, a stored stream of no bytes
// (GHF_E_CORRUPT), a capacity that does not suffice (GHF_E_CAP) -- for its whole workgroup, before the workgroup's first
// store.  Workgroup 0 stores the head and the zero pads of the tables.  The stream region is one run of
// 16-byte vectors cut into contiguous slabs, a slab per workgroup, in the shape of k_stream_copy (16 bytes per lane, four
// loads in flight, non-temporal loads and stores); inside its slab a workgroup walks the sections it covers.  The last
// vector of a stream is masked: what stands in a slot behind its image becomes zero pad.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_tensor_pack(const TensorPackParams P) {
  __shared__ uint64_t s_size[kTensorSlots], s_off[kTensorSlots + 1];
  __shared__ uint64_t s_head[kTensorHeadBytes / 8];
  __shared__ uint32_t s_verdict;
  const uint32_t tid = threadIdx.x;
#pragma unroll
  for (uint32_t j = 0; j < kTensorSlots; ++j)
    if (tid == j) s_size[j] = ((P.stored >> j) & 1u) ? P.stream_bytes[j] : 0ull;
  __syncthreads();
  // ONE lane reads the status word and decides for the whole workgroup: workgroup 0 may latch that very word in this launch,
  // and waves that read it for themselves could disagree on what they saw
  if (tid == 0) {
    uint64_t o = P.streams_off;
    bool empty = false;
    for (uint32_t j = 0; j < kTensorSlots; ++j) {
      s_off[j] = o;
      empty |= ((P.stored >> j) & 1u) && s_size[j] == 0;
      // a size no capacity holds (a slot's size is unspecified behind a failed stage): 16 of them must not wrap the sum
      const uint64_t sz = s_size[j] > (1ull << 58) ? (1ull << 58) : s_size[j];
      o += (sz + 15u) & ~15ull;
    }
    s_off[kTensorSlots] = o;
    s_verdict = *P.status != 0 ? kPackLatched : empty ? kPackEmpty : o > P.cap ? kPackCap : kPackGo;
  }
  __syncthreads();
  const uint64_t total = s_off[kTensorSlots];
  const uint32_t verdict = s_verdict;
  if (verdict != kPackGo) {  // every workgroup reaches its verdict, the same for all its waves, before its first store
    if (blockIdx.x == 0 && tid == 0 && verdict == kPackCap) {
      latch_status(P.status, GHF_E_CAP);
      *P.out_bytes = total;  // the capacity that would have sufficed
    }
    // a stored stream of no bytes is not one any stage writes: its directory entry would be one the parse refuses
    if (blockIdx.x == 0 && tid == 0 && verdict == kPackEmpty) latch_status(P.status, GHF_E_CORRUPT);
    return;  // behind a latched status nothing is stored
  }
  if (blockIdx.x == 0) {
    uint64_t w = 0;
    if (tid == 0) w = kTensorMagic;
    if (tid == 1) w = (uint64_t)kTensorVersion | ((uint64_t)P.elem_bytes << 32);
    if (tid == 2) w = P.n_elems;
    if (tid == 3) w = (uint64_t)P.raw_planes | ((uint64_t)P.sparse_planes << 32);
    if (tid == 4) w = (uint64_t)P.flags;
    if (tid == 5) w = total;
#pragma unroll
    for (uint32_t p = 0; p < GHF_PLANES_MAX; ++p)
      if (tid == 8 + p) w = P.n_vals[p];
    if (tid >= 16 && tid < 16 + 2 * kTensorSlots) {  // the streams: {0, 0} where the slot is empty
      const uint32_t j = (tid - 16) >> 1;
      if ((P.stored >> j) & 1u) w = (tid & 1u) ? s_size[j] : s_off[j];
    }
#pragma unroll
    for (uint32_t k = 0; k < kTensorFixed; ++k) {  // the tables, as the host laid them out
      if (tid == 16 + 2 * (kTensorSlots + k)) w = P.fixed_off[k];
      if (tid == 17 + 2 * (kTensorSlots + k)) w = P.fixed_bytes[k];
    }
    if (tid < kTensorHeadBytes / 8) s_head[tid] = w;
    __syncthreads();
    if (tid < kTensorHeadBytes / 16) {
      const uint64_t a = s_head[2 * tid], b = s_head[2 * tid + 1];
      reinterpret_cast<uint4*>(P.out)[tid] = make_uint4((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32));
    }
    // a table is a multiple of 8 bytes long: where it is not one of 16, its pad is one zero word
#pragma unroll
    for (uint32_t k = 0; k < kTensorFixed; ++k)
      if (tid == 64 + k && (P.fixed_bytes[k] & 8u)) *reinterpret_cast<uint64_t*>(P.out + P.fixed_off[k] + P.fixed_bytes[k]) = 0ull;
    if (tid == 0) *P.out_bytes = total;
  }
  // the copy: vectors [lo, end) of the stream region are this workgroup's
  const uint64_t region = (total - P.streams_off) >> 4;
  const uint64_t per = (region + gridDim.x - 1) / gridDim.x;
  const uint64_t lo = (uint64_t)blockIdx.x * per;
  const uint64_t end = lo + per < region ? lo + per : region;
  if (lo >= end) return;
  uint4* const dst = reinterpret_cast<uint4*>(P.out + P.streams_off);
  for (uint32_t j = 0; j < kTensorSlots; ++j) {
    const uint64_t sz = s_size[j];
    if (sz == 0) continue;
    const uint64_t o = (s_off[j] - P.streams_off) >> 4, nv = (sz + 15u) >> 4;
    const uint64_t a = lo > o ? lo : o, b = end < o + nv ? end : o + nv;
    if (a >= b) continue;
    const uint4* const src = reinterpret_cast<const uint4*>(P.streams[j]);
    const uint32_t rem = (uint32_t)sz & 15u;
    const uint64_t last = rem ? o + nv - 1 : ~0ull;  // the vector that holds the stream's end, where that is not whole
    auto ld = [&](uint64_t k) -> uint4 {
      const uint4 v = load_stream(src + (k - o));
      return k == last ? keep_bytes(v, rem) : v;
    };
    uint64_t i = a + tid;
    for (; i + 3 * 256 < b; i += 4 * 256) {
      const uint4 v0 = ld(i), v1 = ld(i + 256), v2 = ld(i + 512), v3 = ld(i + 768);
      store_stream(dst + i, v0);
      store_stream(dst + i + 256, v1);
      store_stream(dst + i + 512, v2);
      store_stream(dst + i + 768, v3);
    }
    for (; i < b; i += 256) store_stream(dst + i, ld(i));
  }
}

void launch_tensor_pack(const TensorPackParams& p, uint32_t groups, hipStream_t s) {
  hipLaunchKernelGGL(k_tensor_pack, dim3(groups), dim3(256), 0, s, p);
}

// *dst = value unless the status word is latched: the size of what ghf_tensor_decode decoded, which a decode that stored
// nothing must not report
__global__ void k_tensor_store_size(uint64_t* dst, uint64_t value, const int* status) {
  if (*status == 0) *dst = value;
}
void launch_tensor_store_size(uint64_t* d_dst, uint64_t value, const int* d_status, hipStream_t s) {
  hipLaunchKernelGGL(k_tensor_store_size, dim3(1), dim3(1), 0, s, d_dst, value, d_status);
}

// ------------------------------------------------------------------------------------------------
// k_tensor_open.  ONE launch, one workgroup per stored stream that has a code.  The workgroup parses the image's .crs2
// header where it lies in the container, by the rules of ghf_code_rules.h (section 1) and in the steps of ghf_parse_header,
// and fills codes[slot] as that call would; it holds the 64-byte header of the stream's seek table -- and, for a mask, of its
// plane's rank table -- against what the head implies.  Any failure latches GHF_E_FORMAT and leaves the code zero: no
// decoder builds tables from a zero code.  Nothing outside the sections the host's parse has placed inside the container
// is read: the header's rows only once the header's size is held against the stream's.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_tensor_open(const TensorOpenParams P) {
  __shared__ ghf_code s_code;
  __shared__ uint32_t s_seen[GHF_NSYM];
  __shared__ uint32_t s_used, s_bad;
  __shared__ unsigned long long s_kraft;
  const uint32_t b = blockIdx.x, tid = threadIdx.x;
  const uint8_t* const h = P.container + P.stream_off[b];
  const uint64_t bytes = P.stream_bytes[b];
  uint32_t* const cw = reinterpret_cast<uint32_t*>(&s_code);
  for (uint32_t i = tid; i < sizeof(ghf_code) / 4; i += 256) cw[i] = 0;
  for (uint32_t i = tid; i < GHF_NSYM; i += 256) s_seen[i] = 0;
  if (tid == 0) {
    s_used = GHF_NSYM;
    s_bad = 0;
    s_kraft = 0;
  }
  __syncthreads();
  // the three words that say how long the header is; the same for every thread
  bool ok = bytes >= kHeaderFixedBytes;
  uint32_t min_len = 0, max_len = 0;
  if (ok) {
    min_len = ld_be32(h + 4 * (1 + GHF_NSYM));
    max_len = ld_be32(h + 4 * (2 + GHF_NSYM));
    ok = hdr_shape_ok(ld_be32(h), min_len, max_len, bytes);
  }
  if (ok) {
    for (uint32_t i = tid; i < GHF_NSYM; i += 256) {
      const uint32_t s = ld_be32(h + 4 * (1 + i));
      s_code.symbol[i] = s;
      if (s == kSymUnused) atomicMin(&s_used, i);
    }
    if (tid >= 1 && tid <= max_len) {
      const uint8_t* row = h + 4 * (3 + GHF_NSYM) + 8 * (tid - 1);
      s_code.start_pos[tid] = ld_be32(row);
      s_code.first_code[tid] = ld_be32(row + 4);
    }
  }
  __syncthreads();
  const uint32_t used = s_used;
  if (ok)  // the used symbols are a prefix, all distinct
    for (uint32_t i = tid; i < GHF_NSYM; i += 256) {
      const uint32_t s = s_code.symbol[i];
      if (!hdr_symbol_ok(i, s, used) || (i < used && atomicExch(&s_seen[s], 1u))) atomicOr(&s_bad, 1u);
    }
  __syncthreads();
  ok = ok && !s_bad && s_seen[GHF_NSYM - 1];  // ... the end mark among them
  if (ok && used == 1) {
    if (tid == 0) {
      if (!hdr_lone_end_mark_ok((int)max_len, s_code.start_pos, s_code.first_code)) atomicOr(&s_bad, 1u);
      s_code.length[GHF_NSYM - 1] = 1;
    }
  } else if (ok && tid >= 1 && tid <= max_len) {
    // per-symbol lengths and codewords; the code must be the canonical complete prefix code
    const uint32_t len = tid;
    unsigned long long term;
    if (!hdr_len_ok((int)len, (int)min_len, (int)max_len, used, s_code.start_pos, s_code.first_code, &term)) {
      atomicOr(&s_bad, 1u);
    } else {
      atomicAdd(&s_kraft, term);
      if (len >= min_len) {
        const uint32_t a = s_code.start_pos[len], e = len < max_len ? s_code.start_pos[len + 1] : used;
        for (uint32_t r = 0; r < e - a; ++r) {
          const uint32_t s = s_code.symbol[a + r];
          s_code.length[s] = len;
          s_code.codeword[s] = s_code.first_code[len] + r;
        }
      }
    }
  }
  if (tid == 0) {
    s_code.min_len = (int32_t)min_len;
    s_code.max_len = (int32_t)max_len;
    // the seek table of this stream: what ghf_seek_pack writes for `symbols` symbols of a whole stream
    const uint8_t* const t = P.container + P.table_off[b];
    const uint64_t n = P.symbols[b];
    bool tab = ld_le64(t) == kSeekMagic && ld_le32(t + 8) == kSeekVersion && ld_le32(t + 12) == 0u && ld_le64(t + 16) == n &&
               ld_le32(t + 24) == (uint32_t)kBlockSymbols && ld_le32(t + 28) == (uint32_t)kRunSymbols && ld_le64(t + 32) == blocks_for(n) &&
               (ld_le64(t + 40) | ld_le64(t + 48) | ld_le64(t + 56)) == 0ull;
    if (P.rank_off[b]) {  // a mask: the rank table of its plane
      const uint8_t* const r = P.container + P.rank_off[b];
      const uint64_t nb = (P.n_elems + kSparseRankElems - 1) / kSparseRankElems;
      tab = tab && ld_le64(r) == kSparseRankMagic && ld_le32(r + 8) == kSparseRankVersion && ld_le32(r + 12) == kSparseRankElems &&
            ld_le64(r + 16) == P.n_elems && ld_le64(r + 24) == P.rank_n_vals[b] && ld_le64(r + 32) == nb &&
            (ld_le64(r + 40) | ld_le64(r + 48) | ld_le64(r + 56)) == 0ull;
    }
    if (!tab) atomicOr(&s_bad, 1u);
  }
  __syncthreads();
  if (ok && used != 1 && s_kraft != (1ull << 32)) ok = false;
  if (!ok || s_bad) {
    if (tid == 0) latch_status(P.status, GHF_E_FORMAT);
    return;  // the code stays zero
  }
  uint32_t* const out = reinterpret_cast<uint32_t*>(P.codes + P.slot[b]);
  for (uint32_t i = tid; i < sizeof(ghf_code) / 4; i += 256) out[i] = cw[i];
}

void launch_tensor_open(const TensorOpenParams& p, hipStream_t s) {
  if (p.n_streams) hipLaunchKernelGGL(k_tensor_open, dim3(p.n_streams), dim3(256), 0, s, p);
}

}  // namespace ghf
