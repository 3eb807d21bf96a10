/* include/ghf_tensor.h -- one stored object per typed tensor: the container GHFTENS1.
 * The last section of the C ABI; include/ghf.h includes it at its end, so `#include "ghf.h"` declares everything here.
 * It is a file of its own as golden-huffman_amd/ghf_tensor.py is a module of its own: the binding of ghf.h's own
 * declarations (ghf.py) is a recorded surface that this section does not touch.
 *
 * A tensor stored by ghf_compress_planes_forms is 2 * elem_bytes slots, as many device sizes, codes and side-cars, a rank
 * table per sparse plane, two masks and the value counts -- all of it the caller's to keep.  THE CONTAINER is all of it as
 * ONE contiguous, self-describing, relocatable image, written on the device without a host wait for the sizes, opened from
 * its first GHF_TENSOR_HEAD_BYTES bytes and served by the decoders of sections 23, 25 and 26 unchanged.
 *
 * FORMAT.  Little-endian; every offset counts from byte 0 of the container and is a multiple of 16.
 *   head, 768 bytes:
 *     bytes 0 .. 127: "GHFTENS1", u32 version = 1, u32 elem_bytes, u64 n_elems, u32 raw_planes, u32 sparse_planes, u32 flags,
 *                     u32 0, u64 total_bytes, 16 zero bytes, u64 n_vals[8] (the non-zero bytes of sparse plane p; 0 for
 *                     every other plane).  flags bit 0 = GHF_TENSOR_DELTA: the planes are those of new ^ base.
 *     bytes 128 .. 767: a directory of 40 entries {u64 offset, u64 bytes}: 0 .. 15 the stored stream of slot j (the slot
 *                     order of ghf_compress_planes_forms), 16 .. 31 the seek table of slot j, 32 .. 39 the rank table of
 *                     plane p; an absent section is {0, 0}.
 *   payload from byte 768: the seek tables, j ascending; the rank tables, p ascending; the streams, j ascending.  Each
 *     section starts at a multiple of 16 and is padded with zero bytes to the next; total_bytes is the padded end of the last.
 * Everything whose size the host knows stands in front of everything whose size only the device knows.  No .crs2, seek-table
 * or rank-table byte changes: a dense stream is the standalone .crs2 image, a raw stream the plane, a seek table what
 * ghf_seek_pack writes for that image (start bits from byte 0 of the image), a rank table what ghf_sparse_rank_pack writes.
 *
 * Every device pointer is 16-byte aligned unless said otherwise.  Call-level refusals come before anything touches HIP,
 * with nothing queued, in the order and style of the forms calls of section 23. */
#ifndef GHF_TENSOR_H_
#define GHF_TENSOR_H_
#include "ghf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GHF_TENSOR_HEAD_BYTES 768
#define GHF_TENSOR_DIR_ENTRIES 40
#define GHF_TENSOR_DELTA 1u /* flags bit 0: the planes are those of new ^ base; a decode needs the base */

typedef struct ghf_tensor_section {
  uint64_t offset, bytes; /* {0, 0}: absent */
} ghf_tensor_section;

/* the head's fields, and the 40 directory entries */
typedef struct ghf_tensor_info {
  uint32_t version, elem_bytes;
  uint64_t n_elems;
  uint32_t raw_planes, sparse_planes, flags, reserved;
  uint64_t total_bytes;
  uint64_t n_vals[GHF_PLANES_MAX];
  ghf_tensor_section dir[GHF_TENSOR_DIR_ENTRIES];
} ghf_tensor_info;

typedef struct ghf_tensor ghf_tensor; /* an opened container: ghf_tensor_open .. ghf_tensor_close */

/* No reference counterpart (a size the flat buffers of include/compressor.h:62-73 do not need).  Host only: a capacity
 * that suffices for the container of any tensor of n_elems elements of elem_bytes bytes, whatever its forms -- the head,
 * 2 * elem_bytes seek tables, elem_bytes rank tables and 2 * elem_bytes slots of ghf_planes_slot_bytes.  0: elem_bytes is
 * not 2, 4 or 8, or the size overflows. */
size_t ghf_tensor_bound(size_t n_elems, uint32_t elem_bytes);

/* No reference counterpart (the container of what Compressor::compress(), include/compressor.h:62-73, writes per stored
 * stream).  What ghf_compress_planes_forms left -- h_stream_ptrs (HOST [2 * elem_bytes] device pointers: the slots, each
 * readable to its stream's size rounded up to 16), d_stream_bytes (DEVICE u64 [2 * elem_bytes]: its d_out_bytes),
 * h_indexes (HOST [2 * elem_bytes]: the live side-cars), h_rank_ptrs (HOST [elem_bytes] DEVICE rank-table images; may be
 * NULL without sparse planes), the masks and h_n_vals as it reported them -- becomes the container at d_container[0 ..
 * cap).  NEVER synchronises.  Queued: ghf_seek_pack per stream that has a code, straight into the container; a copy per
 * rank table; then ONE launch, k_tensor_pack, in which every workgroup forms the exclusive scan of the padded device
 * sizes itself (no workgroup waits for another), workgroup 0 stores the head, and all workgroups copy the stream region in
 * contiguous slabs; the last vector of a stream is masked, so the pads are zero whatever the slots held.
 * *d_container_bytes (DEVICE u64) <- total_bytes.  total_bytes > cap: GHF_E_CAP is latched, *d_container_bytes still
 * receives the size that would have sufficed, and the launch stores nothing else; nothing at or beyond cap is ever
 * written.  A stored stream whose device size is 0 is not one any stage writes (its directory entry would be one
 * ghf_tensor_parse refuses): GHF_E_CORRUPT is latched and nothing is stored.  The verdict -- a latched status, such a size,
 * the capacity -- is formed by one lane per workgroup, for all its waves, before the workgroup's first store.  Behind a
 * latched status the launch stores nothing.
 * Refused, in this order: a null context, h_stream_ptrs, d_stream_bytes, h_indexes, h_n_vals, d_container or
 * d_container_bytes; elem_bytes not 2, 4 or 8; a sparse_planes or raw_planes bit at or above elem_bytes, an AUTO, a plane
 * in both masks; unknown flags; a sparse plane with h_n_vals[p] > n_elems; a stored stream whose pointer is null or
 * misaligned, a misaligned d_container, a d_stream_bytes or d_container_bytes that is not 8-byte aligned, a sparse plane
 * without its rank table; n_elems * elem_bytes beyond size_t; a side-car that does not cover exactly the symbols of its
 * stream: GHF_E_INVAL; n_elems == 0: GHF_E_EMPTY; cap below the host-known part (head, seek tables, rank tables):
 * GHF_E_CAP. */
int ghf_tensor_pack(ghf_ctx* ctx, const uint8_t* const* h_stream_ptrs /* HOST [2 * elem_bytes] */,
                    const uint64_t* d_stream_bytes /* DEVICE [2 * elem_bytes] */, const ghf_index* h_indexes /* [2 * elem_bytes] */,
                    const uint8_t* const* h_rank_ptrs /* HOST [elem_bytes] DEVICE images, or NULL */, unsigned raw_planes,
                    unsigned sparse_planes, const size_t* h_n_vals /* [elem_bytes] */, size_t n_elems, uint32_t elem_bytes,
                    unsigned flags, uint8_t* d_container, size_t cap, uint64_t* d_container_bytes);

/* No reference counterpart: Compressor::compress(), include/compressor.h:62-73, for a typed tensor, into one container.
 * ghf_compress_planes_forms and ghf_tensor_pack in one call: the slots, side-cars and rank slots are workspaces of the
 * context that grow on demand (the side-cars of all streams are views into one pair of arrays: nothing is allocated per
 * stream).  d_base is optional; with it the planes are those of d_in ^ d_base and the head carries GHF_TENSOR_DELTA.
 * raw_planes / sparse_planes: bits, or GHF_RAW_AUTO / GHF_SPARSE_AUTO.  The call waits for the device exactly as often as
 * ghf_compress_planes_forms does for the same masks: AT MOST ONCE, and NEVER with both masks explicit and no sparse plane.
 * Refusals: those of ghf_compress_planes_forms, in its order, under this call's name; then those of ghf_tensor_pack.  With
 * an AUTO mask the host-known part is known only behind the one wait: a cap below it is then refused with the planes'
 * work queued and nothing written to d_container.
 * DEVICE MEMORY: the workspaces stay with the context behind the call -- 2 * elem_bytes slots of ghf_planes_slot_bytes of
 * n_elems, about 2.25 times the tensor (2.4 GB behind one call on 1 GiB of fp32), beside the plane workspaces of the forms
 * call -- and are reused by the next call; ghf_tensor_workspace_release gives them back, ghf_ctx_destroy frees them. */
int ghf_compress_tensor(ghf_ctx* ctx, const uint8_t* d_in, const uint8_t* d_base /* optional */, size_t n_elems, uint32_t elem_bytes,
                        unsigned raw_planes, unsigned sparse_planes, uint8_t* d_container, size_t cap, uint64_t* d_container_bytes);

/* No reference counterpart (the reference's objects own no device memory).  Frees the workspaces ghf_compress_tensor grew on
 * this context (slots, rank slots, sizes, pooled side-cars); the next call grows them again.  WAITS for the context's
 * stream first: a pack that is still queued reads the slots.  A null context: GHF_E_INVAL. */
int ghf_tensor_workspace_release(ghf_ctx* ctx);

/* No reference counterpart (validates the container of what Decompressor::decompress(), include/compressor.h:87-92,
 * reads).  Host only, no GPU, nothing queued.  h_head[0 .. head_bytes) is the start of a container of container_bytes
 * bytes; head_bytes >= GHF_TENSOR_HEAD_BYTES.  GHF_E_FORMAT: a wrong magic or version; elem_bytes not 2, 4 or 8; a mask bit
 * at or above elem_bytes; a plane in both masks; unknown flags; non-zero reserved bytes; n_elems == 0 or n_elems *
 * elem_bytes beyond 64 bits; n_vals[p] > n_elems, or non-zero for a plane that is not sparse; an offset that is not a
 * multiple of 16; sections out of the stated order or overlapping; a section or total_bytes beyond container_bytes;
 * total_bytes other than the padded end of the last section; a present or absent section that contradicts the masks and
 * n_vals; a raw stream whose size is not n_elems; a seek table whose size is not ghf_seek_bytes of its stream's symbol
 * count (n_elems, ghf_sparse_mask_bytes of n_elems, or n_vals[p]); a rank table whose size is not ghf_sparse_rank_bytes of
 * n_elems.  A null pointer: GHF_E_INVAL.  *info <- the fields and the directory (zeroed on failure). */
int ghf_tensor_parse(const uint8_t* h_head, size_t head_bytes, size_t container_bytes, ghf_tensor_info* info);

/* No reference counterpart (opens the container for Decompressor::decompress(), include/compressor.h:87-92).  First the
 * rules of ghf_tensor_parse on h_head (HOST, head_bytes >= GHF_TENSOR_HEAD_BYTES): on failure the call returns at once,
 * queues nothing, and *out = NULL.  Then the handle: a zeroed device array of 2 * elem_bytes codes and ONE launch,
 * k_tensor_open, one workgroup per stored stream that has a code: it checks that image's .crs2 header on the device by the
 * rules of ghf_parse_header and fills the stream's code as that call would, and holds the 64-byte headers of the stream's
 * seek table and (for a mask) of its plane's rank table against what the head implies.  A failure latches GHF_E_FORMAT
 * and leaves the code zero: every decoder then refuses it.  No byte outside d_container[0 .. container_bytes) is read,
 * whatever the head says.  The call waits for the device ONLY when a plane is sparse, to bring its rank tables to the
 * host for the range call; a table that ghf_sparse_rank_parse refuses, or that counts other values than the head:
 * GHF_E_FORMAT, *out = NULL.  h_head == NULL is allowed: the call then fetches the 768 bytes itself, and waits for them.
 * d_container must stay where it is, unchanged, while the handle is open; the handle belongs to the context's device. */
int ghf_tensor_open(ghf_ctx* ctx, const uint8_t* h_head, size_t head_bytes, const uint8_t* d_container, size_t container_bytes,
                    ghf_tensor** out);

/* No reference counterpart (the reference's objects own no device memory).  Frees the handle's codes and host tables; the
 * container itself is the caller's.  Work queued on the handle must have finished (ghf_sync).  NULL: GHF_OK. */
int ghf_tensor_close(ghf_tensor* t);

/* No reference counterpart (the reference's streams do not describe themselves).  Host only: *info <- what the head of the
 * opened container said. */
int ghf_tensor_describe(const ghf_tensor* t, ghf_tensor_info* info);

/* No reference counterpart: Decompressor::decompress(), include/compressor.h:87-92, for the whole tensor of an opened
 * container.  A thin driver: ghf_decode_planes_forms_range from the container's seek tables over the range [0, n_elems),
 * then *d_out_bytes (optional, DEVICE u64) <- n_elems * elem_bytes, unless a status is latched: behind a latched status
 * neither d_out nor *d_out_bytes is written.  Everything that call promises carries over: its
 * refusals, d_base == d_out, nothing stored behind a latched status, NO wait.  d_base is the whole base tensor.  A
 * container with GHF_TENSOR_DELTA and no d_base, or a d_base for a container without the flag: GHF_E_INVAL, nothing
 * queued. */
int ghf_tensor_decode(ghf_ctx* ctx, const ghf_tensor* t, const uint8_t* d_base /* per the flag */, uint8_t* d_out, size_t cap,
                      uint64_t* d_out_bytes /* optional */);

/* No reference counterpart: Decompressor::decompress(), include/compressor.h:87-92, for elements [first, first + count).
 * ghf_decode_planes_forms_range from the container's seek tables; d_base (per the flag, as above) holds the base elements
 * of the range itself, indexed like d_out, and may be d_out.  Never synchronises. */
int ghf_tensor_decode_range(ghf_ctx* ctx, const ghf_tensor* t, const uint8_t* d_base /* per the flag */, uint64_t first,
                            uint64_t count, uint8_t* d_out, size_t cap);

/* No reference counterpart: Decompressor::decompress(), include/compressor.h:87-92, for many rows in one launch.
 * ghf_decode_planes_gather_forms on the container: row r is elements [d_index[r] * index_stride, + row_elems), d_base (per
 * the flag, as above) is the WHOLE base tensor and must not overlap d_out.  The row caps, the per-row statuses in
 * d_row_status and every refusal are that call's; it never synchronises and never latches the context. */
int ghf_tensor_gather(ghf_ctx* ctx, const ghf_tensor* t, const uint8_t* d_base /* per the flag */, const uint64_t* d_index,
                      uint64_t index_stride, uint32_t row_elems, uint32_t n_rows, uint8_t* d_out, size_t out_stride,
                      int32_t* d_row_status);

#ifdef __cplusplus
}
#endif
#endif /* GHF_TENSOR_H_ */
