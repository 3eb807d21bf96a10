// golden-huffman_amd/csrc/ghf_build_code.h -- K2 + K3 as a device-side body, shared by k_build_code (ghf_kernels.hip: one
// wavefront per launch, counts from the 257-entry histogram in global memory) and k_compress_batch (ghf_batch.hip: wave 0 of
// every workgroup, counts from the workgroup's LDS bins).  One wavefront executes it; the caller owns the LDS it works in.
#ifndef GHF_BUILD_CODE_H_
#define GHF_BUILD_CODE_H_
#include <type_traits>

#include "ghf_device.h"

namespace ghf {

// ------------------------------------------------------------------------------------------------
// K2 + K3: code lengths and canonical assignment on one wavefront.
//
// The reference keeps symbol INDICES in a std::priority_queue ordered by the live frequency table
// (include/canonical_huff_encoder.h:58-70).  Which of several equal-weight nodes is popped first is
// decided by libstdc++'s heap layout, and that decides the code lengths, so the heap is emulated
// step for step (lane 0: __push_heap / __adjust_heap as in <bits/stl_heap.h>).  The "+1 for every
// member of both chains" walks of canonical_huff_encoder.cc:316-329 become a recorded merge tree whose
// leaf depths all 64 lanes read off in parallel afterwards.
// ------------------------------------------------------------------------------------------------
// Heap entry = (frequency << 9) | symbol index in ONE 64-bit word, so a sift level moves one word and a
// parent's two children (and its four grandchildren) are one (two) aligned 16-byte LDS reads.
// The reference's comparator looks at the frequency only -- equal frequencies must compare EQUAL, the
// index must not break ties: comp(a, b) = freq[a] > freq[b]  <=>  ea > (eb | 511).
// Heap position p lives in slot p + 1 so that the child pair (2p+1, 2p+2) sits on a 16-byte boundary.
struct HeapLds {
  alignas(16) unsigned long long slot[528];
  uint16_t parent[GHF_NSYM + 256 + 7];  // Huffman tree: node -> parent node (0 = none); leaves 0..256, merges 257..
  uint16_t cur[GHF_NSYM + 3];           // symbol index kept in the heap -> the tree node it currently stands for
};

typedef unsigned long long u64t;
struct alignas(16) U64x2 { u64t x, y; };

__device__ __forceinline__ bool heap_gt(u64t a, u64t b) { return a > (b | 511ull); }  // freq(a) > freq(b)

__device__ __forceinline__ void heap_sift_up(HeapLds& h, int hole, u64t e) {
  // libstdc++ __push_heap(first, hole, top = 0, value, comp)
  while (hole > 0) {
    const int parent = (hole - 1) >> 1;
    const u64t pe = h.slot[parent + 1];
    if (!heap_gt(pe, e)) break;
    h.slot[hole + 1] = pe;
    hole = parent;
  }
  h.slot[hole + 1] = e;
}

// std::pop_heap + pop_back: a[0] leaves, then __adjust_heap(first, 0, len = n-1, value = old back): the hole
// walks to the bottom always taking the child for which comp(right, left) is false -> right, else left (two
// levels per LDS round trip: the grandchildren are fetched together with the children), the lone left
// child of an even-length heap is handled, then the displaced value is pushed up from the hole.
__device__ __forceinline__ u64t heap_pop(HeapLds& h, int& n) {
  const u64t top = h.slot[1];
  const int len = n - 1;
  n = len;
  if (len < 1) return top;
  const u64t value = h.slot[len + 1];
  int hole = 0;
  const int lim = (len - 1) >> 1;
  while (hole < lim) {
    const U64x2 c = *reinterpret_cast<const U64x2*>(&h.slot[2 * hole + 2]);   // positions 2h+1, 2h+2
    const U64x2 g0 = *reinterpret_cast<const U64x2*>(&h.slot[4 * hole + 4]);  // positions 4h+3, 4h+4
    const U64x2 g1 = *reinterpret_cast<const U64x2*>(&h.slot[4 * hole + 6]);  // positions 4h+5, 4h+6
    const bool left = heap_gt(c.y, c.x);
    const int child = 2 * hole + (left ? 1 : 2);
    h.slot[hole + 1] = left ? c.x : c.y;
    hole = child;
    if (hole < lim) {
      const U64x2 g = left ? g0 : g1;
      const bool left2 = heap_gt(g.y, g.x);
      const int child2 = 2 * hole + (left2 ? 1 : 2);
      h.slot[hole + 1] = left2 ? g.x : g.y;
      hole = child2;
    }
  }
  if ((len & 1) == 0 && hole == ((len - 2) >> 1)) {
    const int child = 2 * (hole + 1);
    h.slot[hole + 1] = h.slot[child];  // position child - 1
    hole = child - 1;
  }
  heap_sift_up(h, hole, value);
  return top;
}

// ---- the same two heap operations, executed by the WHOLE wave in a constant number of steps ----
// A sift only ever touches one root-to-leaf path, and libstdc++'s __adjust_heap picks that path from
// sibling comparisons alone (the value being re-inserted plays no part until the final __push_heap).  With
// 1-based node numbers t (slot[t]; children 2t and 2t+1 sit on one 16-byte boundary), lane l OWNS the
// children of nodes l and 64 + l (lane 0: nodes 128 and 64) -- 128 parents cover a heap of 257 entries:
//   1. ONE LDS round trip: every lane loads the children pairs of its two nodes; root and last entry are
//      read along.  Two ballots = a 128-bit map "preferred child is the right one" for the whole heap;
//   2. the scalar unit follows the map from the root down: t = 2t + bit[t], two or three scalar
//      instructions a level, no memory;
//   3. everything the pop has to move is ALREADY in registers: the entry that moves up into path node u is
//      u's preferred child, held by u's owner.  Every lane checks whether its nodes are on the path
//      (t_leaf >> shift == u), one ballot against the re-inserted value tells where __push_heap stops, and
//      the owners store: slot[u] = child entry above the stop, slot[stop] = value.
// Identical result to the sequential code above in a third of its time; heap_pop/heap_sift_up stay as the
// executable specification.
__device__ __forceinline__ u64t wave_uniform(u64t x) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)x);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(x >> 32));
  return ((u64t)hi << 32) | lo;
}

__device__ __forceinline__ u64t lane_above(u64t x) {  // value held by lane + 1 (same row of 16 lanes)
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)x, 0x101, 0xF, 0xF, false);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(x >> 32), 0x101, 0xF, 0xF, false);
  return ((u64t)hi << 32) | lo;
}

__device__ __forceinline__ u64t wave_heap_pop(HeapLds& h, int& n, int lane) {
  const int len = __builtin_amdgcn_readfirstlane(n) - 1;  // entries left behind (wave-uniform: keeps the walk on the scalar unit)
  n = len;
  const uint32_t tA = lane ? (uint32_t)lane : 128u, tB = 64u + (uint32_t)lane;
  // (all four reads go out together and are waited for once: a pop is two LDS round trips, this one and the path's below)
  const U64x2 ca = *reinterpret_cast<const U64x2*>(&h.slot[2 * tA]);
  const U64x2 cb = *reinterpret_cast<const U64x2*>(&h.slot[2 * tB]);
  const u64t top_v = h.slot[1];
  const u64t value_v = h.slot[len + 1];  // (len == 0: slot[1] again, unused)
  __builtin_amdgcn_sched_barrier(0);
  const u64t top = wave_uniform(top_v);
  if (len < 1) return top;
  const u64t value = wave_uniform(value_v);  // the old last entry, re-inserted from the hole
  // 1. "go right" = !comp(right, left) (libstdc++ takes the LEFT child when freq[right] > freq[left])
  const unsigned long long R0 = __ballot(!heap_gt(ca.y, ca.x));  // bit l = node l (l >= 1), bit 0 = node 128
  const unsigned long long R1 = __ballot(!heap_gt(cb.y, cb.x));  // bit l = node 64 + l
  // 2. walk.  0-based: while (hole < (len - 1) / 2) -> child; 1-based t = hole + 1: while (t <= lim).  With D = depth of
  //    the last position, every node above depth D-1 has two children: the first D-1 steps need no bounds test.
  const uint32_t lim = (uint32_t)(len - 1) >> 1;
  const int D = 31 - __clz(len);
  // seven levels unconditionally (two scalar instructions each), then cut the path back to its first D-1 steps: the
  // prefix of a longer walk IS the shorter walk (what lies below may be stale slots; it is shifted out)
  // (t = 2 t + bit t of the map: s_bitcmp1_b64 puts the bit into SCC -- it looks at the low six bits of t only, which is
  //  what level 7 wants -- and s_addc_u32 t, t, t adds it in: 14 scalar instructions for the 7 levels; the compiler's
  //  shift / and / shift / or rendering of the same took 40)
  uint32_t t = 1;
  asm("s_bitcmp1_b64 %1, %0\n\ts_addc_u32 %0, %0, %0\n\t"
      "s_bitcmp1_b64 %1, %0\n\ts_addc_u32 %0, %0, %0\n\t"
      "s_bitcmp1_b64 %1, %0\n\ts_addc_u32 %0, %0, %0\n\t"
      "s_bitcmp1_b64 %1, %0\n\ts_addc_u32 %0, %0, %0\n\t"
      "s_bitcmp1_b64 %1, %0\n\ts_addc_u32 %0, %0, %0\n\t"
      "s_bitcmp1_b64 %1, %0\n\ts_addc_u32 %0, %0, %0\n\t"  // nodes 1..63
      "s_bitcmp1_b64 %2, %0\n\ts_addc_u32 %0, %0, %0"        // nodes 64..127
      : "+s"(t)
      : "s"(R0), "s"(R1)
      : "scc");
  const int steps = D - 1 > 0 ? D - 1 : 0;
  t >>= 7 - steps;
  if (t <= lim) t = 2u * t + (uint32_t)(((t < 64u || t == 128u ? R0 : R1) >> (t & 63u)) & 1ull);  // depth D-1 where both children exist
  t <<= (((uint32_t)len & 1u) ^ 1u) & (uint32_t)(t == ((uint32_t)len >> 1));  // lone left child of an even-length heap (kept in scalar arithmetic)
  const int k = 31 - __clz(t);  // depth of the hole
  // 3. lane j < k takes path node u_j = t >> (k - j): ONE more LDS read (the children pair of u_j) gives cv_j, the entry that
  //    __adjust_heap moves up into u_j (its preferred child, which is path node u_{j+1}).  __push_heap from the hole then moves
  //    entries back down while comp(entry, value); it stops below the DEEPEST path entry with !comp: with m = that depth + 1
  //    (0: none), u_i receives cv_i for i < m, u_m receives `value`, everything deeper keeps what it had.
  const uint32_t sh = (uint32_t)(k - lane) & 31u;
  const bool onp = lane < k;
  const uint32_t u = onp ? (t >> sh) : 1u;
  const U64x2 c = *reinterpret_cast<const U64x2*>(&h.slot[2 * u]);
  const u64t cv = ((t >> ((sh - 1u) & 31u)) & 1u) ? c.y : c.x;
  const unsigned long long S = __ballot(!heap_gt(cv, value)) & ((1ull << k) - 1ull);  // lanes 0..k-1 are on the path
  const int m = S ? 64 - __clzll((long long)S) : 0;
  if (lane <= m) h.slot[lane < m ? u : (t >> ((uint32_t)(k - m) & 31u))] = lane < m ? cv : value;
  wave_sync();  // the next heap operation reads, in OTHER lanes, what these lanes stored (without the fence the compiler may
                // forward a lane's own store to its next load and let the other lanes' load overtake the store)
  return top;
}

// priority_queue::push(e) onto a heap of n entries: __push_heap from position n.  In two steps, so that a caller can put
// other LDS reads into the same round trip: lane j = 1..depth reads the j-th ancestor of the new position ...
struct PushLoad {
  u64t pe;
  int aj, depth;
  bool on;
};
__device__ __forceinline__ PushLoad wave_heap_push_load(const HeapLds& h, int n_, int lane) {
  const int n = __builtin_amdgcn_readfirstlane(n_);
  PushLoad L;
  L.depth = 31 - __clz(n + 1);  // number of ancestors of position n
  L.on = lane >= 1 && lane <= L.depth;
  L.aj = ((n + 1) >> lane) - 1;  // lane 0: n itself
  L.pe = L.on ? h.slot[L.aj + 1] : 0ull;
  return L;
}
// ... and the entries above the first ancestor that stays move down one level each (one ballot, one DPP shift)
__device__ __forceinline__ void wave_heap_push_finish(HeapLds& h, const PushLoad& L, u64t e, int lane) {
  const bool stop = L.on && !heap_gt(L.pe, e);
  const unsigned long long sm = __ballot(stop);
  const int t = sm ? (__ffsll((long long)sm) - 1) - 1 : L.depth;  // entries of lanes 1..t move down one level
  const u64t up = lane_above(L.pe);
  if (lane <= t) h.slot[L.aj + 1] = (lane < t) ? up : e;
  wave_sync();
}
__device__ __forceinline__ void wave_heap_push(HeapLds& h, int n_, u64t e, int lane) {
  const PushLoad L = wave_heap_push_load(h, n_, lane);
  wave_heap_push_finish(h, L, e, lane);
}

struct CodeLds {  // the small per-length tables of K3; the per-symbol arrays go straight to global memory
  uint32_t num[40];
  uint32_t first_code[64];
  uint32_t start_pos[64];
  int32_t min_len, max_len;
};

// SURVEY 8(f) N4, opt-in (GHF_CODE_LIMIT): where the reference cannot go (a code longer than 32 bits,
// include/canonical_huff_encoder.h:43-44) the lengths are replaced by the optimal 32-bit-limited ones
// (package-merge; definition and tie rules: oracle/huff_oracle.c orc_limit_lengths).  Rare and small (<= 257 leaves,
// 32 levels): ranking is done by all lanes, the merges by lane 0.
struct LimitLds {
  unsigned long long w[2][2 * GHF_NSYM];
  uint8_t is_leaf[33][2 * GHF_NSYM];
  uint16_t order[GHF_NSYM + 3];
  uint16_t len_of[34], taken[34];
  uint32_t newlen[GHF_NSYM + 3];
  long long freq[GHF_NSYM + 3];
  int n;
};

__device__ void limit_lengths_32(LimitLds& Q, const uint32_t (&len)[5], int lane) {
  constexpr int kLimit = 32;
  const long long* freq = Q.freq;
  // order: present symbols by (frequency ascending, index ascending)
  if (lane == 0) Q.n = 0;
  __syncthreads();
#pragma unroll 1
  for (int j = 0; j < 5; ++j) {
    const int s = lane + 64 * j;
    if (s >= GHF_NSYM || len[j] == 0) continue;
    const long long f = freq[s];
    int rank = 0;
    for (int t = 0; t < GHF_NSYM; ++t) {
      const long long g = freq[t];
      rank += (g != 0) && (g < f || (g == f && t < s));
    }
    Q.order[rank] = (uint16_t)s;
    atomicAdd(&Q.n, 1);
  }
  __syncthreads();
  if (lane == 0) {
    const int n = Q.n;
    int prev_n = 0, cur = 0;
    for (int d = kLimit; d >= 1; --d) {
      const unsigned long long* pw = Q.w[cur ^ 1];
      unsigned long long* cw = Q.w[cur];
      const int npk = prev_n / 2;
      int li = 0, pi = 0, k = 0;
      while (li < n || pi < npk) {
        const unsigned long long lw = li < n ? (unsigned long long)freq[Q.order[li]] : ~0ull;
        const unsigned long long pk = pi < npk ? pw[2 * pi] + pw[2 * pi + 1] : ~0ull;
        if (li < n && (pi >= npk || lw <= pk)) {
          cw[k] = lw;
          Q.is_leaf[d][k] = 1;
          ++li;
        } else {
          cw[k] = pk;
          Q.is_leaf[d][k] = 0;
          ++pi;
        }
        ++k;
      }
      Q.len_of[d] = (uint16_t)k;
      prev_n = k;
      cur ^= 1;
    }
    int need = 2 * n - 2;
    for (int d = 1; d <= kLimit; ++d) {
      if (need > (int)Q.len_of[d]) need = Q.len_of[d];
      int leaves = 0;
      for (int k = 0; k < need; ++k) leaves += Q.is_leaf[d][k];
      Q.taken[d] = (uint16_t)leaves;
      need = 2 * (need - leaves);
    }
  }
  __syncthreads();
  for (int i = lane; i < GHF_NSYM; i += 64) Q.newlen[i] = 0;
  __syncthreads();
  for (int i = lane; i < Q.n; i += 64) {
    uint32_t l = 0;
    for (int d = 1; d <= kLimit; ++d) l += i < (int)Q.taken[d];
    Q.newlen[Q.order[i]] = l;
  }
  __syncthreads();
}

// LIMIT = the GHF_CODE_LIMIT instantiation: it alone carries LimitLds (26 KiB).  The default one stays small enough
// in LDS to be scheduled next to the streaming kernels of a pipelined caller instead of waiting for a CU to drain.
struct NoLimitLds {};

// A point every lane of the building wave passes before any of them goes on.  ONE_WAVE_GROUP: the wave is its whole
// workgroup (k_build_code), so the workgroup barrier is that point.  Otherwise the other waves of the workgroup are
// waiting somewhere else and must not be met here: the wave's own in-order LDS / memory pipeline is enough.
template <bool ONE_WAVE_GROUP>
__device__ __forceinline__ void code_sync() {
  if constexpr (ONE_WAVE_GROUP) __syncthreads();
  else wave_sync();
}

// The counts' domain (include/ghf.h, ghf_build_code): a heap entry has 64 - 9 = GHF_HIST_TOTAL_BITS bits for a node's
// weight and the root's weight is the sum of all counts, so that sum must stay below 2^55.  `mine` = the sum of this lane's
// counts, `any_big` = one of them is 2^55 or more by itself (with none that big, a sum of 257 cannot wrap 64 bits).
// Registers only: one ballot, one wave reduction, one compare.  Wave-uniform result.
__device__ __forceinline__ bool counts_out_of_domain(u64t mine, bool any_big) {
  if (__ballot(any_big)) return true;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d, 64);
  return (mine >> GHF_HIST_TOTAL_BITS) != 0;
}

struct HistCounts {  // the counts as K1 leaves them: u64[257] in global memory (k_build_code, k_build_codes)
  static constexpr bool kAnyCount = true;  // caller-supplied 64-bit counts: held to the domain before the first push
  const unsigned long long* __restrict__ hist;
  __device__ __forceinline__ long long operator()(int s) const { return (long long)hist[s]; }
};

// The body.  counts(s) = the count of symbol s (0..256; the end mark's is 1), as a long long; Counts::kAnyCount says
// whether their sum can reach 2^55 at all (else the domain check is compiled out).  Failures (GHF_E_INVAL for counts out
// of the domain, GHF_E_EMPTY, GHF_E_CODELEN) are latched at *status -- the context's status word, or a word of the
// caller's own -- and end the body; *out is then not (completely) written.  s_ndata: one LDS int.
template <bool LIMIT, bool ONE_WAVE_GROUP, class QLds, class Counts>
__device__ __forceinline__ void build_code_body(HeapLds& heap, QLds& Q, CodeLds& cl, int& s_ndata, const Counts counts,
                                                ghf_code* __restrict__ out, int* __restrict__ status, uint32_t empty_ok,
                                                const int lane) {
  // the 257 counts live in registers (lane l holds symbols l, l + 64, ..): LDS is kept under 7 KiB so that this wave
  // fits on a CU next to K7's 153 KiB (or K5's, or K1's) instead of waiting for one of their workgroups to retire
  long long fr[5];
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const int s = lane + 64 * j;
    fr[j] = s < GHF_NSYM ? counts(s) : 0ll;
    if constexpr (LIMIT) {
      if (s < GHF_NSYM) Q.freq[s] = fr[j];
    }
  }
  if constexpr (Counts::kAnyCount) {
    u64t mine = 0;
    bool any_big = false;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      mine += (u64t)fr[j];
      any_big |= ((u64t)fr[j] >> GHF_HIST_TOTAL_BITS) != 0;
    }
    if (counts_out_of_domain(mine, any_big)) {  // a weight would wrap in the heap word: refused, *out untouched
      if (lane == 0) latch_status(status, GHF_E_INVAL);
      return;
    }
  }
  for (int s = lane; s < GHF_NSYM; s += 64) heap.cur[s] = (uint16_t)s;
  for (int i = lane; i < GHF_NSYM + 256 + 7; i += 64) heap.parent[i] = 0;
  if (lane < 40) cl.num[lane] = 0;
  cl.first_code[lane] = 0;
  cl.start_pos[lane] = 0;
  code_sync<ONE_WAVE_GROUP>();

  // ---- K2: get_encoding_length, canonical_huff_encoder.cc:289-345.  The ORDER of heap operations is strictly
  // sequential (which of several equal-weight nodes pops first is decided by the heap layout), but each single
  // operation is done by all 64 lanes at once; the merges are recorded as a tree and the depths read off later.
  {
    int n = 0, ndata = 0;
    for (int s = 0; s < GHF_NSYM; ++s) {  // .cc:301-306: ascending index, zero counts skipped
      const u64t f = (u64t)__shfl(fr[s >> 6], s & 63, 64);  // wave-uniform: readlane
      if (f) {
        wave_heap_push(heap, n, (f << 9) | (u64t)s, lane);  // priority_queue::push
        ++n;
        if (s < 256) ++ndata;
      }
    }
    if (lane == 0) s_ndata = ndata;
    const int times = n - 1;  // .cc:309
    for (int t = 0; t < times; ++t) {
      const u64t e1 = wave_heap_pop(heap, n, lane);  // .cc:311-314
      const u64t e2 = wave_heap_pop(heap, n, lane);
      const int s1 = (int)(e1 & 511u), s2 = (int)(e2 & 511u);
      const int node = GHF_NSYM + t;
      // one LDS round trip for the push's ancestors and the two groups' current tree nodes (every lane reads the same
      // two words: no divergent block, no wait of its own)
      const PushLoad pl = wave_heap_push_load(heap, n, lane);
      const uint16_t g1 = heap.cur[s1], g2 = heap.cur[s2];
      if (lane == 0) {
        heap.parent[g1] = (uint16_t)node;  // .cc:316-329: both groups one level deeper ...
        heap.parent[g2] = (uint16_t)node;
        heap.cur[s2] = (uint16_t)node;     // ... and merged under the second popped index
      }
      const u64t f = (e1 >> 9) + (e2 >> 9);                              // .cc:331
      wave_heap_push_finish(heap, pl, (f << 9) | (u64t)s2, lane);        // .cc:333
      ++n;
    }
  }
  code_sync<ONE_WAVE_GROUP>();
  if (s_ndata == 0 && !empty_ok) {  // empty input: undefined in the reference
    if (lane == 0) latch_status(status, GHF_E_EMPTY);
    return;
  }
  // code length = depth of the leaf; symbols owned by this lane: s_j = lane + 64 j (s = 256 is lane 0, j = 4)
  uint32_t len[5], node[5];
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    len[j] = 0;
    node[j] = (uint32_t)(lane + 64 * j);
    if (node[j] >= GHF_NSYM) node[j] = GHF_NSYM + 256 + 1;  // parent == 0 there
  }
  for (int step = 0; step < 256; ++step) {
    bool any = false;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const uint32_t p = heap.parent[node[j]];
      if (p) {
        node[j] = p;
        len[j] += 1;
        any = true;
      }
    }
    if (!__ballot(any)) break;
  }
  // GHF_EMPTY_OK: the lone end mark (no merge happened, its depth is 0) gets the one-bit code "0" -- our definition
  if (s_ndata == 0 && lane == 0) len[4] = 1;
  uint32_t mx = 0;
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    if (lane + 64 * j >= GHF_NSYM) len[j] = 0;  // lanes past symbol 256 own nothing
    mx = len[j] > mx ? len[j] : mx;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t o = __shfl_xor(mx, d, 64);
    mx = o > mx ? o : mx;
  }
  int max_len = (int)mx;  // .cc:343
  if (max_len > 32) {     // include/canonical_huff_encoder.h:43-44: the reference cannot write such codes
    if constexpr (!LIMIT) {
      if (lane == 0) latch_status(status, GHF_E_CODELEN);
      return;
    } else {
      limit_lengths_32(Q, len, lane);
      mx = 0;
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        const int s = lane + 64 * j;
        len[j] = s < GHF_NSYM ? Q.newlen[s] : 0u;
        mx = len[j] > mx ? len[j] : mx;
      }
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t o = __shfl_xor(mx, d, 64);
        mx = o > mx ? o : mx;
      }
      max_len = (int)mx;
    }
  }

  // ---- K3: do_gen_encode, canonical_huff_encoder.cc:69-141 ----
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const int s = lane + 64 * j;
    if (s < GHF_NSYM) {
      out->length[s] = len[j];
      out->codeword[s] = 0;
      out->symbol[s] = 0xFFFFFFFFu;  // .cc:88
      if (len[j]) atomicAdd(&cl.num[len[j]], 1u);  // .cc:85-87
    }
  }
  code_sync<ONE_WAVE_GROUP>();  // (also orders the symbol[] defaults above before the slots written below)
  const uint32_t num = (lane >= 1 && lane <= max_len) ? cl.num[lane] : 0u;
  const unsigned long long nzmask = __ballot(num != 0);
  const int min_len = __ffsll((long long)nzmask) - 1;                 // .cc:93-98
  const uint32_t spos = wave_incl_scan_u32(num) - num;          // .cc:104-105 start_pos[i] = sum num[1..i-1]
  if (lane >= 1 && lane <= max_len) cl.start_pos[lane] = spos;
  if (lane == 0) {                                                     // .cc:109-121
    uint32_t fc = 0;
    cl.first_code[max_len] = 0;
    for (int i = max_len - 1; i >= 1; --i) {
      fc = (fc + cl.num[i + 1]) >> 1;
      cl.first_code[i] = fc;
    }
    for (int i = 1; i < min_len; ++i) cl.first_code[i] = 1024;
    out->min_len = min_len;
    out->max_len = max_len;
  }
  code_sync<ONE_WAVE_GROUP>();
  out->first_code[lane] = cl.first_code[lane];  // 64 entries each, zero beyond max_len
  out->start_pos[lane] = cl.start_pos[lane];
  // .cc:127-133: within a length, codes and symbol_[] slots go to symbols in ascending index order.
  // rank = (#same-length symbols in earlier 64-symbol rows) + (#same-length lanes below me in my row)
  uint32_t seen = 0;  // lane L holds how many symbols of length L were ranked so far
  for (int j = 0; j < 5; ++j) {
    for (int L = min_len; L <= max_len; ++L) {
      const bool m = (len[j] == (uint32_t)L);
      const unsigned long long mask = __ballot(m);
      if (mask == 0) continue;
      const uint32_t before = __shfl(seen, L, 64);
      if (m) {
        const uint32_t r = before + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        const int s = lane + 64 * j;
        out->codeword[s] = cl.first_code[L] + r;
        out->symbol[cl.start_pos[L] + r] = (uint32_t)s;
      }
      if (lane == L) seen += (uint32_t)__popcll(mask);
    }
  }
}

}  // namespace ghf
#endif
