// golden-huffman_amd/csrc/ghf_gather_core.h -- the run walker of the gather kernels (ghf_planes_gather.hip, DESIGN.md section 25;
// ghf_planes_gather_forms.hip, section 26), gfx950 / wave64: one lane takes one run of 512 symbols of a seekable .crs2
// stream, from the bit its block's record gives, into an LDS stage.  Written once; both units include it.
#ifndef GHF_GATHER_CORE_H_
#define GHF_GATHER_CORE_H_
#include "ghf_batch_core.h"

namespace ghf {

struct GatherLds {  // static; the stage follows as dynamic LDS
  CodeTab t;  // the tables of the plane in work
  CodeVetLds vet;
  int err;
};

// One lane takes run run0 + t of the plane, t < nruns: run k = R % 8 of block g = R / 8 of the seek table (g < n_blocks: the row
// lies inside the n symbols the table was held against on the host).  Checked before an address is formed: the block's
// start_bit + the sum of its run_bits lies inside the stream, and equals the next record's start_bit where there is one.
// Then the run is decoded once, 16 symbols per ds_write_b128 as in batch_decode_runs, into stage bytes [512 t, 512 t + 512),
// and must use exactly its recorded bits; a window that starts no code, or an end mark, fails it too.  Any failure raises
// S.err.  Start bits are 64-bit: the cursor, which counts in 32 bits, is opened on the 16-byte vector that holds the run's
// first bit and sees the stream from there on, so it counts at most 127 + 512 * 32 bits.  No byte outside stream[0 ..
// stream_bytes) or outside the n_blocks records is read.  Every lane of the workgroup calls it with the same arguments; S.t
// holds the filled tables (a barrier lies behind batch_code_tables).
__device__ __forceinline__ void gather_decode_runs(GatherLds& S, uint32_t* stage, const uint8_t* stream, uint64_t stream_bytes,
                                                   const uint8_t* records, uint64_t n_blocks, uint64_t n, uint64_t run0, uint32_t nruns,
                                                   int lb, int long_from, int max_len) {
  // run t goes to lane t / 4 of wave t % 4: the nine runs of a row of 4096 elements then sit in all four waves, whose stream
  // loads -- one dependent load per 32 stream bits, nothing else in flight -- overlap; in one wave they would queue up
  const uint32_t t = ((uint32_t)threadIdx.x & 63u) * (uint32_t)kBatchWaves + ((uint32_t)threadIdx.x >> 6);
  if (t >= nruns) return;
  const uint64_t R = run0 + t, g = R >> 3;
  const uint32_t k = (uint32_t)R & 7u;
  const uint64_t* const rec = reinterpret_cast<const uint64_t*>(records) + g * (kSeekRecordBytes / 8);
  const uint64_t start = rec[0], w0 = rec[1], w1 = rec[2];
  // the eight u16 run lengths lie in w0 (runs 0 .. 3) and w1: the runs in front of run k are the fields below bit 16 k of
  // the pair.  Masks and field sums, no compare per run: k is the lane's own for every plane of the row, and eight pairs of
  // lane masks kept across the plane loop cost more scalar registers than the kernel has
  auto fields = [](uint64_t x) { return (uint32_t)(x & 0xFFFFu) + (uint32_t)((x >> 16) & 0xFFFFu) + (uint32_t)((x >> 32) & 0xFFFFu) + (uint32_t)(x >> 48); };
  const uint32_t sh = 16u * (k & 3u);
  const uint64_t below = (1ull << sh) - 1ull;  // the fields in front of field k & 3 of a word
  const uint32_t before = k < 4u ? fields(w0 & below) : fields(w0) + fields(w1 & below);
  const uint32_t mine = (uint32_t)((k < 4u ? w0 : w1) >> sh) & 0xFFFFu;
  const uint32_t total = fields(w0) + fields(w1);
  const uint64_t end_bit = stream_bytes * 8;
  bool bad = start > end_bit || total > end_bit - start;
  if (g + 1 < n_blocks && rec[3] - start != (uint64_t)total) bad = true;  // the block ends where the next one starts
  if (!bad) {
    const uint64_t sym0 = R * kRunSymbols;  // < n: the row touches the run
    const uint32_t cnt = n - sym0 < (uint64_t)kRunSymbols ? (uint32_t)(n - sym0) : (uint32_t)kRunSymbols;
    const uint64_t B = start + before, skip = (B >> 7) << 4;  // B <= end_bit: skip <= stream_bytes
    const uint8_t* const s = stream + skip;
    const uint64_t bytes = stream_bytes - skip;
    BatchCursor cur;
    cur.seek(s, bytes, (uint32_t)(B & 127u));
    uint32_t used = 0;
    uint4* const out = reinterpret_cast<uint4*>(stage + t * (kRunSymbols / 4));
    const uint32_t ngroups = (cnt + 15u) >> 4;  // groups of 16 symbols: one ds_write_b128 each, zeros behind symbol cnt - 1
#pragma unroll 1
    for (uint32_t gq = 0; gq < ngroups && !bad; ++gq) {
      uint4 q = make_uint4(0, 0, 0, 0);  // the group's four words of symbols, oldest first
#pragma unroll 1
      for (uint32_t w = 0; w < 4u; ++w) {
        uint32_t word = 0;
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) {
          if (16u * gq + 4u * w + i < cnt) {
            const uint32_t ent = batch_decode_one(S.t, cur.window(), lb, long_from, max_len);
            const uint32_t sym = ent & 0x1FFu, len = ent >> 9;
            if (len == 0 || sym == 256u) bad = true;  // no code starts with these bits, or an end mark among the data
            used += len;
            word |= (sym & 0xFFu) << (8u * i);
            cur.skip(s, bytes, len);
          }
        }
        q = make_uint4(q.y, q.z, q.w, word);
      }
      out[gq] = q;
    }
    if (used != mine) bad = true;  // the run does not land on its recorded end
  }
  if (bad) S.err = 1;
}

}  // namespace ghf
#endif
