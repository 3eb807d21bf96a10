"""ctypes binding of lib/libghf.so (C ABI: include/ghf.h).  Plumbing for tests and bench.py: device
memory comes from torch tensors, work is queued on torch's current stream, nothing is computed here.
Loading fails loudly when the HIP library is missing -- there is no CPU fallback in the product."""
import ctypes as C
import os

NSYM = 257
EMIT_LAST = 1
EMIT_REBASE = 2
EMIT_HEADER = 4
EMIT_LONG_CODES = 8  # GHF_EMIT_LONG_CODES: the tables may hold codes of 33..64 bits (a .crs tree deeper than 32)
INDEX_NO_END_MARK = 1
CODE_LIMIT = 1
BATCH_MAX_ITEM = 1 << 20  # GHF_BATCH_MAX_ITEM: the largest item of ghf_compress_batch / ghf_decode_batch
HIST_COVER_ALL = 1  # GHF_HIST_COVER_ALL (ghf_histogram_batch): every count of 0 becomes 1
PLANES_MAX = 8  # GHF_PLANES_MAX: the widest element of the byte-plane calls
PLANES_ELEM_BYTES = (2, 4, 8)
# ghf_internal.h planes_tile_elems / kPlanesGroups: the elements one wave of k_planes_split / k_planes_merge moves at a time
# (tests/test_planes_cpu.py holds them against the kernels' LDS tiles), and the one-wave workgroups of one resident round.
# Tests size their ragged and second-round cases with them; nothing in the library's behaviour depends on them.
PLANES_TILE = {2: 2048, 4: 1024, 8: 1024}
PLANES_GROUPS = 256 * 16
# ghf_internal.h kPlanesHistGroups / kPlanesHistTileVecs * 16 / kPlanesHistFlushTiles: the persistent workgroups of
# k_histogram_planes, the bytes of one of its tiles, and the tiles between two flushes of a workgroup's u32 counters (tests
# size their second-round and past-the-flush cases with them; tests/test_planes_coded_cpu.py holds them against the source)
PLANES_HIST_GROUPS = 256 * 4
PLANES_HIST_TILE_BYTES = 16384
PLANES_HIST_FLUSH_TILES = 3
PLANES_BUILD_CODES = 1  # GHF_PLANES_BUILD_CODES (ghf_compress_planes_coded): d_codes is filled from the tensor's own counts
# ghf_internal.h kSparseTile / kSparseGroups: the bytes of the string one wave of the ghf_sparse.hip kernels takes at a time,
# and the one-wave workgroups of one resident round (beyond SPARSE_TILE * SPARSE_GROUPS bytes a workgroup takes more than one
# tile).  The scan takes one count per workgroup and so never more than ONE step of SPARSE_SCAN counts.  Tests stand on these
# edges (tests/test_sparse_cpu.py holds them against the source); nothing in the library's behaviour depends on them.
SPARSE_TILE = 4096
SPARSE_GROUPS = 256 * 16
SPARSE_SCAN = SPARSE_GROUPS
SPARSE_RANK_ELEMS = 32768  # GHF_SPARSE_RANK_ELEMS: the elements of a rank block: 4096 mask bytes, one seek block
RAW_AUTO = 0x80000000  # GHF_RAW_AUTO (ghf_compress_planes_forms): a plane whose image would be at least n_elems bytes is stored raw
GATHER_MAX_ROW_ELEMS = 32768  # GHF_GATHER_MAX_ROW_ELEMS: the longest row of ghf_decode_planes_gather
GATHER_SPARSE_MAX_ROW_ELEMS = 8192  # GHF_GATHER_SPARSE_MAX_ROW_ELEMS: ... of ghf_decode_planes_gather_forms with a sparse plane
SPARSE_AUTO = 0x80000000  # GHF_SPARSE_AUTO (ghf_compress_planes_sparse): planes with at least 3/4 zero bytes are stored sparse
EMPTY_OK = 2  # opt-in: n == 0 -> header of the one-symbol code + 0x7F (builder's definition, parity unpinned)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libghf.so")

STATUS = {0: "ok", 1: "invalid argument", 2: "HIP error / no device", 3: "empty input", 4: "code longer than 32 bits",
          5: "output capacity too small", 6: "not a .crs2 / .crs header", 7: "corrupt stream", 8: "out of memory",
          9: "one distinct byte value (.crs)", 10: "a byte value without a code in the shared code"}


class GhfError(RuntimeError):
    def __init__(self, status, where, detail=""):
        self.status = status
        super().__init__("%s: ghf status %d (%s) %s" % (where, status, STATUS.get(status, "?"), detail))


class Code(C.Structure):
    """ghf_code == the tables of CanonicalHuffEncoder (reference include/canonical_huff_encoder.h:107-120)."""

    _fields_ = [
        ("length", C.c_uint32 * NSYM),
        ("codeword", C.c_uint32 * NSYM),
        ("symbol", C.c_uint32 * NSYM),
        ("first_code", C.c_uint32 * 64),
        ("start_pos", C.c_uint32 * 64),
        ("min_len", C.c_int32),
        ("max_len", C.c_int32),
    ]

    def as_dict(self):
        ml = self.max_len
        return {
            "length": list(self.length),
            "codeword": list(self.codeword),
            "symbol": list(self.symbol),
            "first_code": list(self.first_code)[1 : ml + 1],
            "start_pos": list(self.start_pos)[1 : ml + 1],
            "min_len": self.min_len,
            "max_len": ml,
        }


class Index(C.Structure):
    _fields_ = [
        ("n_symbols", C.c_uint64),
        ("chunk_symbols", C.c_uint32),
        ("seg_symbols", C.c_uint32),
        ("n_chunks", C.c_uint64),
        ("n_segs", C.c_uint64),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32),
        ("d_chunk_bit", C.c_void_p),
        ("d_seg_bit", C.c_void_p),
    ]


class BatchIndex(C.Structure):
    """ghf_batch_index: the side-cars of a batch, item i's slice at i * blocks_per_item / i * segs_per_item"""

    _fields_ = [
        ("count", C.c_uint32),
        ("reserved", C.c_uint32),
        ("max_item_bytes", C.c_uint64),
        ("blocks_per_item", C.c_uint64),
        ("segs_per_item", C.c_uint64),
        ("d_chunk_bit", C.c_void_p),
        ("d_seg_bit", C.c_void_p),
    ]


class SeekInfo(C.Structure):
    """ghf_seek_info: what ghf_seek_parse reads from the 64-byte header of a seek table"""

    _fields_ = [("n_symbols", C.c_uint64), ("n_blocks", C.c_uint64), ("flags", C.c_uint32), ("version", C.c_uint32)]


class SparseRankInfo(C.Structure):
    """ghf_sparse_rank_info: what ghf_sparse_rank_parse reads from a rank table"""

    _fields_ = [("n", C.c_uint64), ("n_vals", C.c_uint64), ("n_blocks", C.c_uint64), ("version", C.c_uint32), ("reserved", C.c_uint32)]


class Tree(C.Structure):
    """ghf_tree == the reference's HuffTree for the .crs format (include/huff_tree.h:98-176): node ids 0..255 are
    leaves (the key), 256 + i is the i-th parent, left[i] / right[i] its children."""

    _fields_ = [
        ("left", C.c_uint16 * 256),
        ("right", C.c_uint16 * 256),
        ("root", C.c_uint32),
        ("n_leaves", C.c_uint32),
        ("max_len", C.c_uint32),
        ("tree_bytes", C.c_uint32),
        ("header", C.c_uint8 * 1024),
    ]

    def code_strings(self):
        """the 256 root-to-leaf paths as '0'/'1' strings ('' for absent keys) -- NormalHuffEncoder::encode_map_"""
        out = [""] * 256
        stack = [(self.root, "")]
        while stack:
            node, path = stack.pop()
            if node < 256:
                out[node] = path
            else:
                stack.append((self.right[node - 256], path + "1"))
                stack.append((self.left[node - 256], path + "0"))
        return out


# ---- the prototypes of the C ABI: every exported function once, name -> (restype or None for the default int, argtypes).
# lib() applies the table and EXPORTS is its keys, so a name cannot be exported without a prototype.
_vp, _sz, _u64, _i32, _u32, _ui, _str = C.c_void_p, C.c_size_t, C.c_uint64, C.c_int, C.c_uint32, C.c_uint, C.c_char_p
_pvp, _psz, _pu64, _pi32, _pui = C.POINTER(_vp), C.POINTER(_sz), C.POINTER(_u64), C.POINTER(_i32), C.POINTER(_ui)
_pidx, _pbidx, _pseek, _prank = C.POINTER(Index), C.POINTER(BatchIndex), C.POINTER(SeekInfo), C.POINTER(SparseRankInfo)
# ctx, stream pointers, stream sizes, codes, side-cars: the front of every plane decode; a range decode adds the seek tables
# (infos, table pointers, table sizes), one from sparse planes the rank tables (infos, host pointers)
_PLANES_FRONT = [_vp, _pvp, _psz, _vp, _pidx]
_RANGE_FRONT = _PLANES_FRONT + [_pseek, _pvp, _psz]
_SPARSE_RANGE_FRONT = _RANGE_FRONT + [_prank, _pvp]
_COMPRESS_SPARSE = [_vp, _vp, _sz, _u32, _ui, _vp, _sz, _vp, _vp, _pidx, _pui, _psz]
_COMPRESS_SPARSE_DELTA = [_vp, _vp, _vp, _sz, _u32, _ui, _vp, _sz, _vp, _vp, _pidx, _pui, _psz]
_PROTOS = {
    "ghf_ctx_create": (None, [_i32, _pvp]),
    "ghf_ctx_destroy": (None, [_vp]),
    "ghf_ctx_set_stream": (None, [_vp, _vp]),
    "ghf_sync": (None, [_vp]),
    "ghf_status": (None, [_vp]),
    "ghf_clear_status": (None, [_vp]),
    "ghf_last_error": (_str, [_vp]),
    "ghf_status_string": (_str, [_i32]),
    "ghf_version": (None, []),
    "ghf_device_alloc": (None, [_vp, _sz, _pvp]),
    "ghf_device_free": (None, [_vp, _vp]),
    "ghf_host_alloc": (None, [_vp, _sz, _pvp]),
    "ghf_host_free": (None, [_vp, _vp]),
    "ghf_copy_h2d": (None, [_vp, _vp, _vp, _sz]),
    "ghf_copy_d2h": (None, [_vp, _vp, _vp, _sz]),
    "ghf_memset_d": (None, [_vp, _vp, _i32, _sz]),
    "ghf_histogram": (None, [_vp, _vp, _sz, _vp]),
    "ghf_build_code": (None, [_vp, _vp, _vp]),
    "ghf_write_header": (None, [_vp, _vp, _vp, _sz]),
    "ghf_header_bytes": (_sz, [_i32]),
    "ghf_encode_plan": (None, [_vp, _vp, _sz, _vp, _vp]),
    "ghf_encode_emit": (None, [_vp, _vp, _sz, _vp, _vp, _i32, _vp, _sz, _pidx, _vp]),
    "ghf_compress": (None, [_vp, _vp, _sz, _vp, _sz, _vp, _vp, _pidx]),
    "ghf_compress_bound": (_sz, [_sz]),
    "ghf_chunk_symbols": (_u32, [_sz]),
    "ghf_index_alloc": (None, [_vp, _sz, _pidx]),
    "ghf_index_free": (None, [_vp, _pidx]),
    "ghf_parse_header": (None, [_vp, _sz, C.POINTER(Code), _psz]),
    "ghf_decode": (None, [_vp, _vp, _sz, _vp, _pidx, _vp, _sz, _vp]),
    "ghf_decoded_size": (None, [_vp, _vp, _sz, _vp, _pu64]),
    "ghf_shard_start_bit": (None, [_vp, _vp, _vp, _i32, _i32, _vp]),
    "ghf_crs_build_code": (None, [_vp, _vp, _vp, _vp]),
    "ghf_crs_compress": (None, [_vp, _vp, _sz, _vp, _sz, _vp, _vp, _pidx]),
    "ghf_crs_compress_bound": (_sz, [_sz]),
    "ghf_crs_parse_header": (None, [_vp, _sz, C.POINTER(Tree), _psz]),
    "ghf_crs_decode": (None, [_vp, _vp, _sz, _i32, _vp, _pidx, _vp, _sz, _vp]),
    "ghf_crs_decoded_size": (None, [_vp, _vp, _sz, _i32, _vp, _pu64]),
    "ghf_build_code_ex": (None, [_vp, _vp, _vp, _ui]),
    "ghf_compress_ex": (None, [_vp, _vp, _sz, _vp, _sz, _vp, _vp, _pidx, _ui]),
    "ghf_sync_piece": (None, [_vp, _vp, _sz, _u32, _u64, _vp, _pu64, _pu64, _pi32]),
    "ghf_decode_prepare": (None, [_vp, _vp]),
    "ghf_comm_unique_id": (None, [_str]),
    "ghf_comm_init_rank": (None, [_vp, _str, _i32, _i32, _pvp]),
    "ghf_comm_destroy": (None, [_vp]),
    "ghf_comm_world": (None, [_vp, _pi32, _pi32]),
    "ghf_rccl_version": (None, [_pi32]),
    "ghf_comm_allreduce_hist": (None, [_vp, _vp, _vp]),
    "ghf_comm_allgather_total": (None, [_vp, _vp, _vp, _vp]),
    "ghf_encode_sharded": (None, [_vp, _vp, _vp, _sz, _vp, _sz, _vp, _pidx, _vp, _vp]),
    "ghf_shard_bound": (_sz, [_sz]),
    "ghf_event_create": (None, [_vp, _pvp]),
    "ghf_event_destroy": (None, [_vp]),
    "ghf_event_record": (None, [_vp, _vp]),
    "ghf_event_wait": (None, [_vp, _vp]),
    "ghf_event_sync": (None, [_vp]),
    "ghf_histogram_add": (None, [_vp, _vp, _sz, _vp]),
    "ghf_crs_sync_piece": (None, [_vp, _vp, _sz, _u32, _u64, _vp, _pu64, _pu64]),
    "ghf_copy_d2d": (None, [_vp, _vp, _vp, _sz, _i32]),
    "ghf_shard_bytes": (None, [_vp, _vp, _vp, _i32, _i32, _psz]),
    "ghf_seek_bytes": (_sz, [_sz]),
    "ghf_seek_parse": (None, [_vp, _sz, _pseek]),
    "ghf_seek_pack": (None, [_vp, _pidx, _vp, _sz, _vp, _sz]),
    "ghf_seek_expand": (None, [_vp, _pseek, _vp, _sz, _vp, _sz, _vp, _pidx]),
    "ghf_decode_range": (None, [_vp, _vp, _sz, _vp, _pidx, _pseek, _vp, _sz, _u64, _u64, _vp, _sz]),
    "ghf_compress_batch_bound": (_sz, [_sz]),
    "ghf_batch_index_alloc": (None, [_vp, _u32, _sz, _pbidx]),
    "ghf_batch_index_free": (None, [_vp, _pbidx]),
    "ghf_batch_index_item": (None, [_pbidx, _u32, _sz, _pidx]),
    "ghf_compress_batch": (None, [_vp, _vp, _vp, _sz, _u32, _vp, _vp, _vp, _vp, _pbidx, _vp]),
    "ghf_decode_batch": (None, [_vp, _vp, _vp, _vp, _pbidx, _vp, _u32, _vp, _vp, _vp, _vp]),
    "ghf_decode_images_batch": (None, [_vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp]),
    "ghf_decode_images_batch_stats": (None, [_vp, _vp]),
    "ghf_histogram_batch": (None, [_vp, _vp, _vp, _sz, _u32, _ui, _vp]),
    "ghf_compress_batch_shared_bound": (_sz, [_sz]),
    "ghf_compress_batch_shared": (None, [_vp, _vp, _vp, _sz, _u32, _vp, _vp, _vp, _vp, _pbidx, _vp]),
    "ghf_decode_batch_shared": (None, [_vp, _vp, _vp, _vp, _pbidx, _vp, _u32, _vp, _vp, _vp, _vp]),
    "ghf_decode_bodies_batch_shared": (None, [_vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp]),
    "ghf_planes_slot_bytes": (_sz, [_sz]),
    "ghf_planes_split": (None, [_vp, _vp, _sz, _u32, _vp, _sz]),
    "ghf_planes_merge": (None, [_vp, _vp, _sz, _sz, _u32, _vp]),
    "ghf_compress_planes": (None, [_vp, _vp, _sz, _u32, _vp, _sz, _vp, _vp, _pidx]),
    "ghf_decode_planes": (None, _PLANES_FRONT + [_sz, _u32, _vp, _sz, _vp]),
    "ghf_histogram_batch_planes": (None, [_vp, _vp, _vp, _sz, _u32, _u32, _ui, _vp]),
    "ghf_build_codes": (None, [_vp, _vp, _u32, _vp, _ui]),
    "ghf_compress_batch_planes_shared_bound": (_sz, [_sz, _u32]),
    "ghf_compress_batch_planes_shared": (None, [_vp, _vp, _vp, _sz, _u32, _u32, _vp, _vp, _vp, _vp, _pbidx, _vp]),
    "ghf_decode_batch_planes_shared": (None, [_vp, _vp, _vp, _vp, _pbidx, _vp, _u32, _u32, _vp, _vp, _vp, _vp]),
    "ghf_decode_bodies_batch_planes_shared": (None, [_vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _vp]),
    "ghf_batch_seek_bytes": (_sz, [_sz]),
    "ghf_batch_seek_bound": (_sz, [_sz]),
    "ghf_batch_seek_pack": (None, [_vp, _pbidx, _vp, _u32, _u32, _vp, _vp, _vp, _vp]),
    "ghf_decode_bodies_batch_shared_seek": (None, [_vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp]),
    "ghf_decode_bodies_batch_planes_shared_seek": (None, [_vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _vp]),
    "ghf_planes_merge_range": (None, [_vp, _vp, _sz, _sz, _sz, _u32, _vp]),
    "ghf_decode_planes_range": (None, _RANGE_FRONT + [_u32, _u64, _u64, _vp, _sz]),
    "ghf_histogram_planes": (None, [_vp, _vp, _sz, _u32, _ui, _vp]),
    "ghf_planes_image_bytes": (None, [_vp, _vp, _vp, _u32, _vp]),
    "ghf_compress_planes_coded": (None, [_vp, _vp, _sz, _u32, _vp, _ui, _vp, _sz, _vp, _pidx]),
    "ghf_histogram_planes_delta": (None, [_vp, _vp, _vp, _sz, _u32, _ui, _vp]),
    "ghf_planes_split_delta": (None, [_vp, _vp, _vp, _sz, _u32, _vp, _sz]),
    "ghf_planes_merge_delta": (None, [_vp, _vp, _sz, _vp, _sz, _u32, _vp]),
    "ghf_planes_merge_range_delta": (None, [_vp, _vp, _sz, _vp, _sz, _sz, _u32, _vp]),
    "ghf_compress_planes_delta": (None, [_vp, _vp, _vp, _sz, _u32, _vp, _ui, _vp, _sz, _vp, _pidx]),
    "ghf_decode_planes_delta": (None, _PLANES_FRONT + [_vp, _sz, _u32, _vp, _sz, _vp]),
    "ghf_decode_planes_range_delta": (None, _RANGE_FRONT + [_vp, _u32, _u64, _u64, _vp, _sz]),
    "ghf_sparse_mask_bytes": (_sz, [_sz]),
    "ghf_sparse_split": (None, [_vp, _vp, _sz, _vp, _vp, _sz, _vp]),
    "ghf_sparse_merge": (None, [_vp, _vp, _vp, _sz, _sz, _vp]),
    "ghf_compress_planes_sparse": (None, _COMPRESS_SPARSE),
    "ghf_compress_planes_sparse_delta": (None, _COMPRESS_SPARSE_DELTA),
    "ghf_decode_planes_sparse": (None, _PLANES_FRONT + [_ui, _psz, _sz, _u32, _vp, _sz, _vp]),
    "ghf_decode_planes_sparse_delta": (None, _PLANES_FRONT + [_vp, _ui, _psz, _sz, _u32, _vp, _sz, _vp]),
    "ghf_sparse_rank_bytes": (_sz, [_sz]),
    "ghf_sparse_rank_pack": (None, [_vp, _vp, _sz, _vp, _sz]),
    "ghf_sparse_rank_parse": (None, [_vp, _sz, _prank]),
    "ghf_sparse_merge_at": (None, [_vp, _vp, _vp, _sz, _sz, _sz, _vp]),
    "ghf_compress_planes_sparse_ranked": (None, _COMPRESS_SPARSE + [_vp, _sz]),
    "ghf_compress_planes_sparse_ranked_delta": (None, _COMPRESS_SPARSE_DELTA + [_vp, _sz]),
    "ghf_decode_planes_sparse_range": (None, _SPARSE_RANGE_FRONT + [_ui, _sz, _u32, _u64, _u64, _vp, _sz]),
    "ghf_decode_planes_sparse_range_delta": (None, _SPARSE_RANGE_FRONT + [_vp, _ui, _sz, _u32, _u64, _u64, _vp, _sz]),
    "ghf_planes_split_to": (None, [_vp, _vp, _vp, _sz, _u32, _pvp]),
    "ghf_planes_merge_from": (None, [_vp, _pvp, _vp, _sz, _u32, _vp]),
    "ghf_planes_merge_range_from": (None, [_vp, _pvp, _vp, _sz, _u32, _vp]),
    "ghf_compress_planes_forms": (None, [_vp, _vp, _vp, _sz, _u32, _ui, _ui, _vp, _sz, _vp, _vp, _pidx, _vp, _sz, _pui, _pui, _psz]),
    "ghf_decode_planes_forms": (None, _PLANES_FRONT + [_vp, _ui, _ui, _psz, _sz, _u32, _vp, _sz, _vp]),
    "ghf_decode_planes_forms_range": (None, _SPARSE_RANGE_FRONT + [_vp, _ui, _ui, _sz, _u32, _u64, _u64, _vp, _sz]),
    "ghf_decode_planes_gather": (None, [_vp, _pvp, _psz, _vp, _pseek, _pvp, _psz, _ui, _sz, _u32, _vp, _u64, _u32, _u32, _vp, _sz, _vp]),
    "ghf_decode_planes_gather_forms": (None, [_vp, _pvp, _psz, _vp, _pseek, _pvp, _psz, _prank, _pvp, _psz, _vp, _ui, _ui, _sz, _u32,
                                              _vp, _u64, _u32, _u32, _vp, _sz, _vp]),
    "ghf_batch_planes_raw_auto": (None, [_vp, _vp, _vp, _u32, _vp]),
    "ghf_compress_batch_planes_forms": (None, [_vp, _vp, _vp, _sz, _u32, _u32, _vp, _u32, _vp, _vp, _vp, _pbidx, _vp]),
    "ghf_decode_batch_planes_forms": (None, [_vp, _vp, _vp, _vp, _pbidx, _vp, _u32, _u32, _u32, _vp, _vp, _vp, _vp]),
    "ghf_decode_bodies_batch_planes_forms": (None, [_vp, _vp, _vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp, _vp]),
    "ghf_decode_bodies_batch_planes_forms_seek": (None, [_vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp, _vp]),
}
EXPORTS = list(_PROTOS)
COMM_ID_BYTES = 128

_lib = None


def lib():
    """load libghf.so; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GhfError(2, "load", "libghf.so not built: run `make -C golden-huffman_amd` (or __graft_entry__.build())")
    # One HIP runtime per process: torch ships its own libamdhip64.so (same SONAME as /opt/rocm's).  Import
    # torch FIRST so that libghf.so's DT_NEEDED libamdhip64.so.7 binds to the copy torch already mapped; loading
    # libghf.so first would map /opt/rocm's runtime beside torch's and the second one finds no device.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in _PROTOS.items():
        f = getattr(L, name)
        f.argtypes = argtypes
        if restype is not None:
            f.restype = restype
    _lib = L
    return L


def lib_identity():
    """path and sha256 of the library this process bound (bench.py prints it)"""
    import hashlib

    with open(LIB_PATH, "rb") as f:
        return {"path": os.path.relpath(LIB_PATH, os.path.dirname(_HERE)), "sha256": hashlib.sha256(f.read()).hexdigest()}


def compress_bound(n):
    return int(lib().ghf_compress_bound(n))


def compress_batch_bound(max_item_bytes):
    """capacity that suffices for every item of a batch whose items have at most max_item_bytes"""
    return int(lib().ghf_compress_batch_bound(max_item_bytes))


def compress_batch_shared_bound(max_item_bytes):
    """capacity that suffices for the BODY of every item of a shared-code batch, under any code of <= 32 bits"""
    return int(lib().ghf_compress_batch_shared_bound(max_item_bytes))


def compress_batch_planes_shared_bound(max_item_bytes, elem_bytes):
    """capacity that suffices for every slot (item, plane) of a shared-code batch of elements of elem_bytes bytes"""
    return int(lib().ghf_compress_batch_planes_shared_bound(max_item_bytes, elem_bytes))


def batch_seek_bytes(n_symbols):
    """size of the run record of a shared-code body of n_symbols: 8 + 2 * ceil(n / 128), rounded up to 8"""
    return int(lib().ghf_batch_seek_bytes(n_symbols))


def batch_seek_bound(max_item_bytes):
    """a 16-byte aligned slot that suffices for the run record of every body of up to max_item_bytes symbols"""
    return int(lib().ghf_batch_seek_bound(max_item_bytes))


def planes_slot_bytes(n_elems):
    """a slot that suffices for the image of any byte plane of n_elems elements (a multiple of 16)"""
    return int(lib().ghf_planes_slot_bytes(n_elems))


def sparse_mask_bytes(n):
    """(n + 7) // 8: the bytes of the mask of a byte string of n bytes in the sparse form"""
    return int(lib().ghf_sparse_mask_bytes(n))


def sparse_rank_bytes(n):
    """64 + 8 * (ceil(n / 32768) + 1): the bytes of the rank table of a byte string of n bytes"""
    return int(lib().ghf_sparse_rank_bytes(n))


def sparse_rank_parse(host_bytes):
    """host-side validation of a whole rank table (header, size and every step of cum). -> SparseRankInfo"""
    import numpy as np

    a = np.ascontiguousarray(host_bytes, dtype=np.uint8)
    info = SparseRankInfo()
    rc = lib().ghf_sparse_rank_parse(a.ctypes.data, a.size, C.byref(info))
    if rc:
        raise GhfError(rc, "ghf_sparse_rank_parse")
    return info


def sparse_rank_table(x):
    """the rank table of the byte string x as numpy computes it (for tests): uint8[64 + 8 * (ceil(n / 32768) + 1)]"""
    import numpy as np

    x = np.ascontiguousarray(x, dtype=np.uint8).ravel()
    n = x.size
    nb = -(-n // SPARSE_RANK_ELEMS)
    nz = np.concatenate([[0], np.cumsum(x != 0, dtype=np.uint64)]).astype(np.uint64)
    cum = nz[np.minimum(np.arange(nb + 1, dtype=np.int64) * SPARSE_RANK_ELEMS, n)]
    head = np.zeros(8, dtype="<u8")
    head[0] = int.from_bytes(b"GHFRANK1", "little")
    head[1] = 1 | SPARSE_RANK_ELEMS << 32
    head[2], head[3], head[4] = n, int(nz[n]), nb
    return np.concatenate([head, cum.astype("<u8")]).view(np.uint8)


def batch_index_item(bidx, i, n_i):
    """item i's slice of a BatchIndex as an ordinary Index (a view: it owns nothing); host only"""
    view = Index()
    rc = lib().ghf_batch_index_item(C.byref(bidx), i, n_i, C.byref(view))
    if rc:
        raise GhfError(rc, "ghf_batch_index_item")
    return view


def shard_bound(n):
    """capacity for one shard of a sharded stream (packed with the GLOBAL code: up to 32 bits per symbol)"""
    return int(lib().ghf_shard_bound(n))


def comm_unique_id():
    """ncclGetUniqueId through the C ABI: 128 bytes that rank 0 hands to every rank (any transport)"""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    rc = lib().ghf_comm_unique_id(buf)
    if rc:
        raise GhfError(rc, "ghf_comm_unique_id", "RCCL not available in this process")
    return buf.raw


def rccl_version():
    v = C.c_int(0)
    return v.value if lib().ghf_rccl_version(C.byref(v)) == 0 else None


def chunk_symbols(n):
    return int(lib().ghf_chunk_symbols(n))


def parse_header(host_bytes):
    """host-side header parse + validation (reference canonical_huff_encoder.cc:349-374). -> (Code, header_bytes)"""
    import numpy as np

    a = np.ascontiguousarray(host_bytes, dtype=np.uint8)
    code = Code()
    hs = C.c_size_t(0)
    rc = lib().ghf_parse_header(a.ctypes.data, a.size, C.byref(code), C.byref(hs))
    if rc:
        raise GhfError(rc, "ghf_parse_header")
    return code, hs.value


def seek_bytes(n):
    """size of the seek table of a stream of n symbols: 64 + 24 * ceil(n / 4096)"""
    return int(lib().ghf_seek_bytes(n))


def seek_parse(host_bytes):
    """host-side validation of a seek table's header against the table's size. -> SeekInfo"""
    import numpy as np

    a = np.ascontiguousarray(host_bytes, dtype=np.uint8)
    info = SeekInfo()
    rc = lib().ghf_seek_parse(a.ctypes.data, a.size, C.byref(info))
    if rc:
        raise GhfError(rc, "ghf_seek_parse")
    return info


def crs_parse_header(host_bytes):
    """host-side parse + validation of a .crs tree header (reference include/huff_tree.cc:289-303). -> (Tree, tree_bytes)"""
    import numpy as np

    a = np.ascontiguousarray(host_bytes, dtype=np.uint8)
    tree = Tree()
    tb = C.c_size_t(0)
    rc = lib().ghf_crs_parse_header(a.ctypes.data, a.size, C.byref(tree), C.byref(tb))
    if rc:
        raise GhfError(rc, "ghf_crs_parse_header")
    return tree, tb.value


# ---- marshalling, each step once.  The host arrays made here hold addresses C reads during the call: whoever makes one keeps
# it referenced (an argument of the call, or a local of the method that calls) until the call has returned.
def _addr(x):
    """what C gets for a device buffer: None -> NULL, an int address as it is, a tensor's data_ptr()"""
    return None if x is None else x if isinstance(x, int) else x.data_ptr()


def _ref(struct):
    """byref of a ctypes structure, None -> NULL"""
    return None if struct is None else C.byref(struct)


def _ptr_array(xs, n):
    """a host array of n addresses from the first n of xs: tensors, int addresses or None (-> NULL)"""
    return (C.c_void_p * n)(*[_addr(x) for x in list(xs)[:n]])


def _size_array(values, n):
    """a host size_t array of n entries from the first n of values"""
    return (C.c_size_t * n)(*[int(v) for v in list(values)[:n]])


def _n_elems(d_in, elem_bytes, n_elems):
    """n_elems, by default all of the tensor d_in taken as elements of elem_bytes bytes"""
    return d_in.numel() * d_in.element_size() // elem_bytes if n_elems is None else n_elems


def _seek_tables(infos, d_tables, table_bytes, n):
    """(SeekInfo array, table pointers, table sizes) of n slots, or three NULLs without infos.  A None info is SeekInfo() with
    a table of 0 bytes; table_bytes defaults to seek_bytes(info.n_symbols)."""
    if infos is None:
        return None, None, None
    infos = list(infos)[:n]
    if table_bytes is None:
        table_bytes = [0 if i is None else seek_bytes(i.n_symbols) for i in infos]
    return (SeekInfo * n)(*[SeekInfo() if i is None else i for i in infos]), _ptr_array(d_tables, n), _size_array(table_bytes, n)


def _rank_arrays(ranks, n, device):
    """ranks: None, or per plane None or (SparseRankInfo, table[, table bytes]) -> (infos, pointers, sizes, keep) of n planes
    (NULLs without ranks).  device False: the tables are HOST bytes, and `keep` holds the contiguous arrays the pointers
    point into: the caller keeps it until the call has returned.  device True: tensors or addresses, with their sizes."""
    if ranks is None:
        return None, None, None, []
    infos, ptrs, sizes, keep = (SparseRankInfo * n)(), (C.c_void_p * n)(), (C.c_size_t * n)(), []
    for p, r in enumerate(ranks):
        if r is None:
            continue
        infos[p] = r[0]
        if device:
            ptrs[p] = _addr(r[1])
            sizes[p] = 0 if r[1] is None else r[2] if len(r) > 2 else r[1].numel()
        elif r[1] is not None:
            import numpy as np

            keep.append(np.ascontiguousarray(r[1], dtype=np.uint8))
            ptrs[p] = keep[-1].ctypes.data
    return infos, ptrs, sizes, keep


def _entry(shared, forms, raw):
    """(entry point, what it takes more): without a mask of raw planes (None) the all-dense call `shared`, with one (an int,
    0 included) its twin `forms` and the mask"""
    return (shared, ()) if raw is None else (forms, (raw,))


class Context:
    """one ghf_ctx; work is queued on torch's current stream of `device`."""

    EMIT_LAST = EMIT_LAST
    EMIT_REBASE = EMIT_REBASE
    EMIT_HEADER = EMIT_HEADER
    compress_bound = staticmethod(compress_bound)
    shard_bound = staticmethod(shard_bound)
    parse_header = staticmethod(parse_header)

    def __init__(self, device=0):
        import torch

        self.torch = torch
        self.L = lib()
        self.device = torch.device("cuda", device)
        h = C.c_void_p()
        rc = self.L.ghf_ctx_create(device, C.byref(h))
        if rc:
            raise GhfError(rc, "ghf_ctx_create", self.L.ghf_last_error(None).decode(errors="replace"))
        self.h = h
        self.use_current_stream()

    def use_current_stream(self):
        s = self.torch.cuda.current_stream(self.device).cuda_stream
        self._chk(self.L.ghf_ctx_set_stream(self.h, C.c_void_p(s)), "ghf_ctx_set_stream")

    def use_stream(self, stream):
        """queue on the given torch.cuda.Stream (no change of torch's current stream)"""
        self._chk(self.L.ghf_ctx_set_stream(self.h, C.c_void_p(stream.cuda_stream)), "ghf_ctx_set_stream")

    def close(self):
        if getattr(self, "h", None):
            self.L.ghf_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, where):
        if rc:
            raise GhfError(rc, where, self.L.ghf_last_error(self.h).decode(errors="replace"))

    def _call(self, name, *args):
        """the C function `name` on this context; a status raises GhfError with that name as its `where`"""
        self._chk(getattr(self.L, name)(self.h, *args), name)

    def sync(self):
        """wait for the stream; raises when a device-side stage latched an error."""
        rc = self.L.ghf_sync(self.h)
        if rc:
            self.L.ghf_clear_status(self.h)
            raise GhfError(rc, "ghf_sync", "")

    # ---- tensors -------------------------------------------------------------------------------
    def empty_u8(self, n):
        return self.torch.empty(max(int(n), 1), dtype=self.torch.uint8, device=self.device)

    def new_code(self):
        return self.torch.zeros(C.sizeof(Code), dtype=self.torch.uint8, device=self.device)

    def code_to_host(self, d_code):
        b = d_code.cpu().numpy().tobytes()
        return Code.from_buffer_copy(b)

    def code_to_device(self, code):
        import numpy as np

        a = np.frombuffer(bytes(code), dtype=np.uint8).copy()
        return self.torch.from_numpy(a).to(self.device)

    def copy_d2d(self, d_dst, d_src, n=None, non_temporal=True):
        """the library's streaming copy kernel (bandwidth probe)"""
        n = d_src.numel() if n is None else n
        self._chk(self.L.ghf_copy_d2d(self.h, d_dst.data_ptr(), d_src.data_ptr(), n, 1 if non_temporal else 0), "ghf_copy_d2d")

    # ---- stages --------------------------------------------------------------------------------
    def histogram(self, d_in, n=None, out=None):
        n = d_in.numel() if n is None else n
        hist = self.torch.empty(NSYM, dtype=self.torch.int64, device=self.device) if out is None else out
        self._chk(self.L.ghf_histogram(self.h, d_in.data_ptr(), n, hist.data_ptr()), "ghf_histogram")
        return hist

    def histogram_add(self, d_in, hist, n=None):
        """hist[0..255] += counts of d_in (an input that arrives in pieces); hist[256] = 1"""
        n = d_in.numel() if n is None else n
        self._chk(self.L.ghf_histogram_add(self.h, d_in.data_ptr(), n, hist.data_ptr()), "ghf_histogram_add")
        return hist

    def build_code(self, d_hist, d_code=None, flags=0):
        d_code = self.new_code() if d_code is None else d_code
        if flags:
            self._chk(self.L.ghf_build_code_ex(self.h, d_hist.data_ptr(), d_code.data_ptr(), flags), "ghf_build_code_ex")
        else:
            self._chk(self.L.ghf_build_code(self.h, d_hist.data_ptr(), d_code.data_ptr()), "ghf_build_code")
        return d_code

    def write_header(self, d_code, d_out):
        self._chk(self.L.ghf_write_header(self.h, d_code.data_ptr(), d_out.data_ptr(), d_out.numel()), "ghf_write_header")

    def encode_plan(self, d_in, d_code, n=None, total=None):
        n = d_in.numel() if n is None else n
        if total is None:
            total = self.torch.empty(1, dtype=self.torch.int64, device=self.device)
        self._chk(self.L.ghf_encode_plan(self.h, d_in.data_ptr(), n, d_code.data_ptr(), total.data_ptr()), "ghf_encode_plan")
        return total

    def encode_emit(self, d_in, d_code, d_out, start_bit=None, flags=EMIT_LAST, index=None, n=None, end=None):
        n = d_in.numel() if n is None else n
        if end is None:
            end = self.torch.empty(2, dtype=self.torch.int64, device=self.device)
        self._chk(
            self.L.ghf_encode_emit(self.h, d_in.data_ptr(), n, d_code.data_ptr(),
                                   None if start_bit is None else start_bit.data_ptr(), flags, d_out.data_ptr(),
                                   d_out.numel(), None if index is None else C.byref(index), end.data_ptr()),
            "ghf_encode_emit")
        return end

    def shard_start_bit(self, d_code, d_totals, world, rank, out=None):
        if out is None:
            out = self.torch.empty(1, dtype=self.torch.int64, device=self.device)
        self._chk(self.L.ghf_shard_start_bit(self.h, d_code.data_ptr(), d_totals.data_ptr(), world, rank, out.data_ptr()), "ghf_shard_start_bit")
        return out

    def shard_bytes(self, d_code, d_totals, world, rank):
        """exact size of this rank's shard output, from the all-gathered bit totals (one host synchronisation)"""
        out = C.c_size_t(0)
        self._chk(self.L.ghf_shard_bytes(self.h, d_code.data_ptr(), d_totals.data_ptr(), world, rank, C.byref(out)), "ghf_shard_bytes")
        return int(out.value)

    def index_alloc(self, n):
        idx = Index()
        self._chk(self.L.ghf_index_alloc(self.h, n, C.byref(idx)), "ghf_index_alloc")
        return idx

    def index_free(self, idx):
        self.L.ghf_index_free(self.h, C.byref(idx))

    def index_to_host(self, idx):
        """the side-car's two device arrays as numpy arrays (chunk_bit u64[n_chunks], seg_bit u32[n_segs]); synchronises"""
        import numpy as np

        chunk_bit = np.zeros(idx.n_chunks, dtype=np.uint64)
        seg_bit = np.zeros(idx.n_segs, dtype=np.uint32)
        if chunk_bit.size:
            self._chk(self.L.ghf_copy_d2h(self.h, chunk_bit.ctypes.data, idx.d_chunk_bit, chunk_bit.nbytes), "ghf_copy_d2h")
        if seg_bit.size:
            self._chk(self.L.ghf_copy_d2h(self.h, seg_bit.ctypes.data, idx.d_seg_bit, seg_bit.nbytes), "ghf_copy_d2h")
        self.sync()
        return chunk_bit, seg_bit

    def compress(self, d_in, d_out=None, d_code=None, index=None, n=None, code_flags=0):
        """whole single-GPU pipeline, no host sync. -> (d_out, d_out_bytes[1] int64 device, d_code)"""
        n = d_in.numel() if n is None else n
        if d_out is None:
            d_out = self.empty_u8(compress_bound(n))
        if d_code is None:
            d_code = self.new_code()
        nbytes = self.torch.zeros(1, dtype=self.torch.int64, device=self.device)
        if code_flags:
            self._chk(
                self.L.ghf_compress_ex(self.h, d_in.data_ptr(), n, d_out.data_ptr(), d_out.numel(), nbytes.data_ptr(),
                                       d_code.data_ptr(), None if index is None else C.byref(index), code_flags),
                "ghf_compress_ex")
            return d_out, nbytes, d_code
        self._chk(
            self.L.ghf_compress(self.h, d_in.data_ptr(), n, d_out.data_ptr(), d_out.numel(), nbytes.data_ptr(),
                                d_code.data_ptr(), None if index is None else C.byref(index)),
            "ghf_compress")
        return d_out, nbytes, d_code

    def decode_prepare(self, d_code):
        self._chk(self.L.ghf_decode_prepare(self.h, d_code.data_ptr()), "ghf_decode_prepare")

    def decoded_size(self, d_stream, stream_bytes, d_code):
        n = C.c_uint64(0)
        self._chk(self.L.ghf_decoded_size(self.h, d_stream.data_ptr(), stream_bytes, d_code.data_ptr(), C.byref(n)), "ghf_decoded_size")
        return n.value

    def decode(self, d_stream, stream_bytes, d_code, index=None, d_out=None, cap=None, nbytes=None):
        """index=None: a stream without side-car (e.g. written by the reference); the library rebuilds it on the GPU."""
        if d_out is None:
            d_out = self.empty_u8(index.n_symbols if index is not None else cap)
        if nbytes is None:
            nbytes = self.torch.empty(1, dtype=self.torch.int64, device=self.device)
        self._chk(
            self.L.ghf_decode(self.h, d_stream.data_ptr(), stream_bytes, d_code.data_ptr(),
                              None if index is None else C.byref(index), d_out.data_ptr(), d_out.numel(), nbytes.data_ptr()),
            "ghf_decode")
        return d_out, nbytes

    # ---- batches of small independent streams (one launch per call, per-item status) ------------
    def batch_index_alloc(self, count, max_item_bytes):
        bidx = BatchIndex()
        self._chk(self.L.ghf_batch_index_alloc(self.h, count, max_item_bytes, C.byref(bidx)), "ghf_batch_index_alloc")
        return bidx

    def batch_index_free(self, bidx):
        self.L.ghf_batch_index_free(self.h, C.byref(bidx))

    batch_index_item = staticmethod(batch_index_item)

    def _i64(self, values):
        return self.torch.tensor([int(v) for v in values], dtype=self.torch.int64).to(self.device)

    def _item_arrays(self, items, sizes):
        """(ptrs, sizes) of a list of CUDA uint8 tensors, or of ONE packed tensor cut by `sizes`"""
        if sizes is None:
            return [x.data_ptr() if x.numel() else 0 for x in items], [int(x.numel()) for x in items]
        sizes = [int(v) for v in sizes]
        base, ptrs, at = items.data_ptr(), [], 0
        for v in sizes:
            ptrs.append(base + at)
            at += v
        return ptrs, sizes

    def _batch_in(self, items, sizes, max_item_bytes, elem_bytes=1):
        """the items of a batch call -> (in_ptrs, in_bytes as int64 CUDA tensors, count, max_item_bytes: by default the largest
        item, at least 1, rounded up to whole elements)"""
        ptrs, sizes = self._item_arrays(items, sizes)
        if max_item_bytes is None:
            max_item_bytes = -(-max(max(sizes, default=1), 1) // elem_bytes) * elem_bytes
        return self._i64(ptrs), self._i64(sizes), len(sizes), max_item_bytes

    def _planes_out(self, count, out_stride, d_out):
        """count output slots of out_stride bytes in one uint8 tensor (allocated unless given) -> (d_out, out_ptrs, out_caps)"""
        t = self.torch
        if d_out is None:
            d_out = t.empty(max(count * out_stride, 16), dtype=t.uint8, device=self.device)
        out_ptrs = d_out.data_ptr() + t.arange(count, dtype=t.int64, device=self.device) * out_stride
        return d_out, out_ptrs, t.full((max(count, 1),), out_stride, dtype=t.int64, device=self.device)

    def _item_status(self, count):
        """(out_bytes int64 of zeros, status int32 of -1) for count slots, never empty; callers hand out [:count]"""
        t = self.torch
        return t.zeros(max(count, 1), dtype=t.int64, device=self.device), t.full((max(count, 1),), -1, dtype=t.int32, device=self.device)

    def _compress_batch_io(self, items, sizes, max_item_bytes, elem_bytes, bound, d_out, out_stride, **codes):
        """inputs and outputs of a batch compress call with elem_bytes output slots per item; `codes` is the call's codes under
        the key its dict shows them.  -> (the result dict, the addresses (in_ptrs, in_bytes, out_ptrs, out_caps, out_bytes,
        status) of the tensors the dict keeps)"""
        in_ptrs, in_bytes, count, max_item_bytes = self._batch_in(items, sizes, max_item_bytes, elem_bytes)
        slots = count * elem_bytes
        if out_stride is None:
            out_stride = bound(max_item_bytes)
        d_out, out_ptrs, out_caps = self._planes_out(slots, out_stride, d_out)
        out_bytes, status = self._item_status(slots)
        res = {"out": d_out, "out_stride": out_stride, "out_bytes": out_bytes[:slots], "status": status[:slots], **codes,
               "in_ptrs": in_ptrs, "in_bytes": in_bytes, "out_ptrs": out_ptrs, "out_caps": out_caps, "count": count,
               "max_item_bytes": max_item_bytes, "keep": items}
        return res, tuple(x.data_ptr() for x in (in_ptrs, in_bytes, out_ptrs, out_caps, out_bytes, status))

    def _decode_batch(self, name, stream_ptrs, stream_bytes, d_codes, index, n_items, more, elem_bytes, d_out, out_stride, out_ptrs,
                      out_caps):
        """the batch decodes with the live side-car; `more`: what the entry point takes between the count and the outputs"""
        count = int(n_items.numel())
        if out_ptrs is None:
            if out_stride is None:
                out_stride = (int(index.max_item_bytes) * elem_bytes + 15) & ~15
            d_out, out_ptrs, out_caps = self._planes_out(count, out_stride, d_out)
        out_bytes, status = self._item_status(count)
        self._call(name, stream_ptrs.data_ptr(), stream_bytes.data_ptr(), d_codes.data_ptr(), C.byref(index), n_items.data_ptr(), count,
                   *more, out_ptrs.data_ptr(), out_caps.data_ptr(), out_bytes.data_ptr(), status.data_ptr())
        return {"out": d_out, "out_stride": out_stride, "out_bytes": out_bytes[:count], "status": status[:count],
                "out_ptrs": out_ptrs, "out_caps": out_caps}

    def _two_pass(self, who, count, out, caps):
        """the outputs of a two-pass batch decode, called by the public method `who`.  out None: the sizes pass, no output
        pointers.  Otherwise the decode pass with `caps`: out True allocates slots of the largest cap rounded up to 16 (reads
        caps back: the one host synchronisation), a tensor is cut into count equal slots.
        -> (the result dict, the call's last arguments: out_ptrs, out_caps, out_bytes, status as addresses or NULL)"""
        t = self.torch
        out_bytes, status = self._item_status(count)
        res = {"out_bytes": out_bytes[:count], "status": status[:count]}
        out_ptrs = out_caps = None
        if out is not None:
            if caps is None:
                raise ValueError(who + ": the decode pass needs caps (e.g. the out_bytes of the sizes pass)")
            if out is True:
                out_stride = (int(caps.max().item()) + 15) & ~15 if count else 16
                out = t.empty(max(count * out_stride, 16), dtype=t.uint8, device=self.device)
            else:
                out_stride = int(out.numel()) // max(count, 1)
            out_ptrs = out.data_ptr() + t.arange(count, dtype=t.int64, device=self.device) * out_stride
            out_caps = t.clamp(caps.to(t.int64), max=out_stride).contiguous()
            res.update(out=out, out_stride=out_stride, out_ptrs=out_ptrs, out_caps=out_caps)
        return res, (_addr(out_ptrs), _addr(out_caps), out_bytes.data_ptr(), status.data_ptr())

    def _decode_bodies(self, name, who, front, count, more, out, caps):
        """the two-pass decodes of shared-code bodies: `front` are the CUDA tensors the entry point takes before the count
        (streams, sizes[, records, sizes], codes), `more` what it takes between the count and the outputs"""
        res, outs = self._two_pass(who, count, out, caps)
        self._call(name, *[x.data_ptr() for x in front], count, *more, *outs)
        return res

    def compress_batch(self, items, sizes=None, max_item_bytes=None, d_out=None, out_stride=None, d_codes=None, index=None):
        """items: a list of CUDA uint8 tensors, or ONE packed CUDA uint8 tensor with `sizes` (item i at the sum of the
        sizes before it).  The pointer and size arrays are built on the device; no host synchronisation.  d_out: one
        uint8 tensor holding item i's image at i * out_stride (allocated here unless given).
        -> dict(out, out_stride, out_bytes int64[count], status int32[count], codes uint8[count, sizeof(Code)], in_ptrs,
                in_bytes, out_ptrs, count, max_item_bytes)"""
        t = self.torch
        if d_codes is None:
            count = len(items) if sizes is None else len(sizes)
            d_codes = t.zeros((max(count, 1), C.sizeof(Code)), dtype=t.uint8, device=self.device)
        r, (ip, ib, op, oc, ob, st) = self._compress_batch_io(items, sizes, max_item_bytes, 1, compress_batch_bound, d_out, out_stride,
                                                              codes=d_codes)
        self._call("ghf_compress_batch", ip, ib, r["max_item_bytes"], r["count"], op, oc, ob, d_codes.data_ptr(), _ref(index), st)
        return r

    def decode_batch(self, stream_ptrs, stream_bytes, d_codes, index, n_symbols, d_out=None, out_stride=None, out_ptrs=None,
                     out_caps=None):
        """stream_ptrs / stream_bytes / n_symbols: int64 CUDA tensors [count] (e.g. out_ptrs, out_bytes and in_bytes of
        compress_batch).  Item i is decoded to d_out[i * out_stride ..) unless out_ptrs / out_caps (int64 CUDA tensors) say
        otherwise.  -> dict(out, out_stride, out_bytes int64[count], status int32[count])"""
        return self._decode_batch("ghf_decode_batch", stream_ptrs, stream_bytes, d_codes, index, n_symbols, (), 1, d_out, out_stride,
                                  out_ptrs, out_caps)

    def decode_images_batch(self, stream_ptrs, stream_bytes, out=None, caps=None, codes=False):
        """Standalone .crs2 images and nothing else.  stream_ptrs / stream_bytes: int64 CUDA tensors [count].
        out=None: the sizes pass -> dict(out_bytes int64[count], status int32[count]).
        Otherwise the decode pass: `caps` (int64 CUDA tensor [count], e.g. the out_bytes of the sizes pass) says how much
        room every item gets; out=True allocates one uint8 tensor with item i at i * out_stride, out_stride = the largest
        cap rounded up to 16 (this reads `caps` back: one host synchronisation); a uint8 CUDA tensor is used as it is, cut
        into count equal slots.  codes=True: also the items' tables, uint8[count, sizeof(Code)].
        -> dict(out, out_stride, out_bytes, status[, codes])"""
        t = self.torch
        count = int(stream_bytes.numel())
        res, (op, oc, ob, st) = self._two_pass("decode_images_batch", count, out, caps)
        d_codes = None
        if codes:
            res["codes"] = d_codes = t.zeros((max(count, 1), C.sizeof(Code)), dtype=t.uint8, device=self.device)
        self._call("ghf_decode_images_batch", stream_ptrs.data_ptr(), stream_bytes.data_ptr(), count, op, oc, ob, _addr(d_codes), st)
        return res

    # ---- shared-code batches: one code for the whole batch, an item's output is its body alone ----
    def histogram_batch(self, items, sizes=None, max_item_bytes=None, flags=0, out=None):
        """the byte counts of all items in one int64[257] CUDA tensor (slot 256 = 1), ready for build_code.  items / sizes
        as in compress_batch; flags: HIST_COVER_ALL.  No host synchronisation."""
        in_ptrs, in_bytes, count, max_item_bytes = self._batch_in(items, sizes, max_item_bytes)
        hist = self.torch.empty(NSYM, dtype=self.torch.int64, device=self.device) if out is None else out
        self._call("ghf_histogram_batch", in_ptrs.data_ptr(), in_bytes.data_ptr(), max_item_bytes, count, flags, hist.data_ptr())
        return hist

    def compress_batch_shared(self, items, d_code, sizes=None, max_item_bytes=None, d_out=None, out_stride=None, index=None):
        """compress_batch under the one code `d_code` (e.g. build_code(histogram_batch(items))): item i's BODY goes to
        d_out[i * out_stride ..).  -> dict(out, out_stride, out_bytes int64[count], status int32[count], code, in_ptrs,
        in_bytes, out_ptrs, out_caps, count, max_item_bytes)"""
        r, (ip, ib, op, oc, ob, st) = self._compress_batch_io(items, sizes, max_item_bytes, 1, compress_batch_shared_bound, d_out,
                                                              out_stride, code=d_code)
        self._call("ghf_compress_batch_shared", ip, ib, r["max_item_bytes"], r["count"], d_code.data_ptr(), op, oc, ob, _ref(index), st)
        return r

    def decode_batch_shared(self, stream_ptrs, stream_bytes, d_code, index, n_symbols, d_out=None, out_stride=None, out_ptrs=None,
                            out_caps=None):
        """decode_batch with one code for all items: stream_ptrs / stream_bytes are the bodies (e.g. out_ptrs and
        out_bytes of compress_batch_shared).  -> dict(out, out_stride, out_bytes int64[count], status int32[count])"""
        return self._decode_batch("ghf_decode_batch_shared", stream_ptrs, stream_bytes, d_code, index, n_symbols, (), 1, d_out,
                                  out_stride, out_ptrs, out_caps)

    def decode_bodies_batch_shared(self, stream_ptrs, stream_bytes, d_code, out=None, caps=None):
        """Bodies under the one code `d_code` and nothing else: no side-car, no sizes.  stream_ptrs / stream_bytes: int64
        CUDA tensors [count] (e.g. out_ptrs and out_bytes of compress_batch_shared, or stored bodies copied up).
        out=None: the sizes pass -> dict(out_bytes int64[count], status int32[count]).
        Otherwise the decode pass, with out / caps as in decode_images_batch -> dict(out, out_stride, out_bytes, status,
        out_ptrs, out_caps)"""
        return self._decode_bodies("ghf_decode_bodies_batch_shared", "decode_bodies_batch_shared", (stream_ptrs, stream_bytes, d_code),
                                   int(stream_bytes.numel()), (), out, caps)

    def decode_images_batch_stats(self, d_stats):
        """d_stats: an int64 CUDA tensor [2] that later decode_images_batch and decode_bodies_batch_shared calls add
        {rounds, passes} to; None: off"""
        self._chk(self.L.ghf_decode_images_batch_stats(self.h, None if d_stats is None else d_stats.data_ptr()),
                  "ghf_decode_images_batch_stats")

    # ---- shared-code batches of typed elements: one code per byte plane; slot j = i * elem_bytes + p ----
    def histogram_batch_planes(self, items, elem_bytes, sizes=None, max_item_bytes=None, flags=0, out=None):
        """the byte counts of every byte plane of all items: an int64[elem_bytes, 257] CUDA tensor, ready for build_codes.
        items / sizes (in bytes) as in compress_batch; flags: HIST_COVER_ALL.  No host synchronisation."""
        in_ptrs, in_bytes, count, max_item_bytes = self._batch_in(items, sizes, max_item_bytes, elem_bytes)
        hists = self.torch.empty((elem_bytes, NSYM), dtype=self.torch.int64, device=self.device) if out is None else out
        self._call("ghf_histogram_batch_planes", in_ptrs.data_ptr(), in_bytes.data_ptr(), max_item_bytes, count, elem_bytes, flags,
                   hists.data_ptr())
        return hists

    def build_codes(self, d_hists, d_codes=None, flags=0):
        """d_hists: int64[n, 257] -> uint8[n, sizeof(Code)]: n exact code builds in one launch"""
        n = int(d_hists.numel()) // NSYM
        if d_codes is None:
            d_codes = self.torch.zeros((n, C.sizeof(Code)), dtype=self.torch.uint8, device=self.device)
        self._chk(self.L.ghf_build_codes(self.h, d_hists.data_ptr(), n, d_codes.data_ptr(), flags), "ghf_build_codes")
        return d_codes

    def compress_batch_planes_shared(self, items, d_codes, elem_bytes, sizes=None, max_item_bytes=None, d_out=None, out_stride=None,
                                     index=None, raw_planes=None):
        """compress_batch_shared per byte plane: slot i * elem_bytes + p holds the BODY of plane p of item i under d_codes[p],
        at d_out[slot * out_stride ..).  index: None or batch_index_alloc(count * elem_bytes, max_item_bytes // elem_bytes).
        -> dict(out, out_stride, out_bytes int64[slots], status int32[slots], codes, in_ptrs, in_bytes, out_ptrs, out_caps,
                count, elem_bytes, max_item_bytes, n_elems int64[count])
        raw_planes (None: this call; an int: ghf_compress_batch_planes_forms, see compress_batch_planes_forms)"""
        r, (ip, ib, op, oc, ob, st) = self._compress_batch_io(items, sizes, max_item_bytes, elem_bytes,
                                                              lambda m: compress_batch_planes_shared_bound(m, elem_bytes), d_out,
                                                              out_stride, codes=d_codes)
        name, raw = _entry("ghf_compress_batch_planes_shared", "ghf_compress_batch_planes_forms", raw_planes)
        self._call(name, ip, ib, r["max_item_bytes"], r["count"], elem_bytes, d_codes.data_ptr(), *raw, op, oc, ob, _ref(index), st)
        r.update(elem_bytes=elem_bytes, n_elems=r["in_bytes"] // elem_bytes)
        return r

    def decode_batch_planes_shared(self, stream_ptrs, stream_bytes, d_codes, index, n_elems, elem_bytes, d_out=None, out_stride=None,
                                   out_ptrs=None, out_caps=None, raw_planes=None):
        """the way back with the live side-car: stream_ptrs / stream_bytes int64[count * elem_bytes] (out_ptrs and out_bytes
        of compress_batch_planes_shared), n_elems int64[count].  Item i is decoded to d_out[i * out_stride ..) unless
        out_ptrs / out_caps (bytes) say otherwise.  -> dict(out, out_stride, out_bytes int64[count], status int32[count])"""
        name, raw = _entry("ghf_decode_batch_planes_shared", "ghf_decode_batch_planes_forms", raw_planes)
        return self._decode_batch(name, stream_ptrs, stream_bytes, d_codes, index, n_elems, (elem_bytes,) + raw, elem_bytes, d_out,
                                  out_stride, out_ptrs, out_caps)

    def decode_bodies_batch_planes_shared(self, stream_ptrs, stream_bytes, d_codes, elem_bytes, out=None, caps=None, raw_planes=None):
        """the way back from nothing but the bytes: stream_ptrs / stream_bytes int64[count * elem_bytes].
        out=None: the sizes pass -> dict(out_bytes int64[count] (bytes), status int32[count]).
        Otherwise the decode pass, with out / caps (bytes per item) as in decode_images_batch."""
        name, raw = _entry("ghf_decode_bodies_batch_planes_shared", "ghf_decode_bodies_batch_planes_forms", raw_planes)
        return self._decode_bodies(name, "decode_bodies_batch_planes_shared", (stream_ptrs, stream_bytes, d_codes),
                                   int(stream_bytes.numel()) // elem_bytes, (elem_bytes,) + raw, out, caps)

    # ---- stored shared-code bodies: one run record per body, the persistent form of a slice of a BatchIndex ----
    def batch_seek_pack(self, index, in_bytes, elem_bytes=1, d_rec=None, rec_stride=None):
        """the live side-car of compress_batch_shared (elem_bytes 1) or compress_batch_planes_shared (2, 4, 8) -> one run
        record per body, slot j at d_rec[j * rec_stride ..).  in_bytes: int64[count], the items' sizes in bytes (the
        in_bytes of the compress call).  -> dict(rec, rec_stride, rec_ptrs, rec_caps, rec_bytes int64[slots], status
        int32[slots])"""
        count = int(in_bytes.numel())
        slots = count * elem_bytes
        if rec_stride is None:
            rec_stride = batch_seek_bound(int(index.max_item_bytes))
        d_rec, rec_ptrs, rec_caps = self._planes_out(slots, rec_stride, d_rec)
        rec_bytes, status = self._item_status(slots)
        self._call("ghf_batch_seek_pack", C.byref(index), in_bytes.data_ptr(), count, elem_bytes, rec_ptrs.data_ptr(),
                   rec_caps.data_ptr(), rec_bytes.data_ptr(), status.data_ptr())
        return {"rec": d_rec, "rec_stride": rec_stride, "rec_ptrs": rec_ptrs, "rec_caps": rec_caps, "rec_bytes": rec_bytes[:slots],
                "status": status[:slots]}

    def decode_bodies_batch_shared_seek(self, stream_ptrs, stream_bytes, rec_ptrs, rec_bytes, d_code, out=None, caps=None):
        """Stored bodies under the one code `d_code`, each with its run record: int64 CUDA tensors [count] of pointers and
        sizes.  out=None: the sizes pass (the records' shapes are checked, the streams are not read) -> dict(out_bytes,
        status).  Otherwise the decode pass, with out / caps as in decode_bodies_batch_shared."""
        return self._decode_bodies("ghf_decode_bodies_batch_shared_seek", "decode_bodies_batch_shared_seek",
                                   (stream_ptrs, stream_bytes, rec_ptrs, rec_bytes, d_code), int(stream_bytes.numel()), (), out, caps)

    def decode_bodies_batch_planes_shared_seek(self, stream_ptrs, stream_bytes, rec_ptrs, rec_bytes, d_codes, elem_bytes, out=None,
                                               caps=None, raw_planes=None):
        """the same for the slots of compress_batch_planes_shared: stream_* / rec_* int64[count * elem_bytes]; out / caps
        (bytes per item) as in decode_bodies_batch_planes_shared."""
        name, raw = _entry("ghf_decode_bodies_batch_planes_shared_seek", "ghf_decode_bodies_batch_planes_forms_seek", raw_planes)
        return self._decode_bodies(name, "decode_bodies_batch_planes_shared_seek", (stream_ptrs, stream_bytes, rec_ptrs, rec_bytes, d_codes),
                                   int(stream_bytes.numel()) // elem_bytes, (elem_bytes,) + raw, out, caps)

    # ---- the plane batch calls with raw planes: raw_planes is one int for the batch, bit p = plane p stored as it is ----
    def batch_planes_raw_auto(self, d_hists, d_codes, out=None):
        """d_hists int64[E, 257], d_codes uint8[E, sizeof(Code)] -> an int32[1] CUDA tensor holding the mask of the planes
        that store no more raw than coded (sum hist * length >= 8 * sum hist).  No host synchronisation: int(mask.item())
        when the caller wants it."""
        elem_bytes = int(d_hists.numel()) // NSYM
        mask = self.torch.zeros(1, dtype=self.torch.int32, device=self.device) if out is None else out
        self._chk(self.L.ghf_batch_planes_raw_auto(self.h, d_hists.data_ptr(), d_codes.data_ptr(), elem_bytes, mask.data_ptr()),
                  "ghf_batch_planes_raw_auto")
        return mask

    def compress_batch_planes_forms(self, items, d_codes, elem_bytes, raw_planes, **kw):
        """compress_batch_planes_shared with the planes of raw_planes stored raw: a raw slot holds the plane's n bytes and
        out_bytes[slot] = n.  The dict carries raw_planes too."""
        r = self.compress_batch_planes_shared(items, d_codes, elem_bytes, raw_planes=int(raw_planes), **kw)
        r["raw_planes"] = int(raw_planes)
        return r

    def decode_batch_planes_forms(self, stream_ptrs, stream_bytes, d_codes, index, n_elems, elem_bytes, raw_planes, **kw):
        """decode_batch_planes_shared for the slots of compress_batch_planes_forms"""
        return self.decode_batch_planes_shared(stream_ptrs, stream_bytes, d_codes, index, n_elems, elem_bytes, raw_planes=int(raw_planes),
                                               **kw)

    def decode_bodies_batch_planes_forms(self, stream_ptrs, stream_bytes, d_codes, elem_bytes, raw_planes, out=None, caps=None):
        """decode_bodies_batch_planes_shared for the slots of compress_batch_planes_forms: a raw slot's count is its size"""
        return self.decode_bodies_batch_planes_shared(stream_ptrs, stream_bytes, d_codes, elem_bytes, out=out, caps=caps,
                                                      raw_planes=int(raw_planes))

    def decode_bodies_batch_planes_forms_seek(self, stream_ptrs, stream_bytes, rec_ptrs, rec_bytes, d_codes, elem_bytes, raw_planes,
                                              out=None, caps=None):
        """decode_bodies_batch_planes_shared_seek for the slots of compress_batch_planes_forms: the record pointer and size of
        a raw slot are ignored"""
        return self.decode_bodies_batch_planes_shared_seek(stream_ptrs, stream_bytes, rec_ptrs, rec_bytes, d_codes, elem_bytes, out=out,
                                                           caps=caps, raw_planes=int(raw_planes))

    # ---- byte planes: elements of 2, 4 or 8 bytes, one ordinary .crs2 image per byte position ---------
    # Every call here has a twin against a base tensor (further down).  Both go through one private method that takes the C
    # entry point's name and `base`: () for the plain call, (address or NULL,) for the twin, spliced where the twin takes it --
    # a twin called without a base still reaches ITS entry point, which refuses it.
    planes_slot_bytes = staticmethod(planes_slot_bytes)

    def _planes_split(self, name, d_in, base, elem_bytes, n_elems, d_planes, plane_stride):
        n_elems = _n_elems(d_in, elem_bytes, n_elems)
        if plane_stride is None:
            plane_stride = (n_elems + 255) & ~255
        if d_planes is None:
            d_planes = self.empty_u8(plane_stride * elem_bytes)
        self._call(name, d_in.data_ptr(), *base, n_elems, elem_bytes, d_planes.data_ptr(), plane_stride)
        return d_planes, plane_stride

    def _planes_merge(self, name, d_planes, plane_stride, base, which, n, elem_bytes, d_out):
        """which: (n_elems,) of a whole merge or (first, count) of a range; n: the elements d_out gets"""
        if d_out is None:
            d_out = self.empty_u8(n * elem_bytes)
        self._call(name, d_planes.data_ptr(), plane_stride, *base, *which, elem_bytes, d_out.data_ptr())
        return d_out

    def _histogram_planes(self, name, d_in, base, elem_bytes, n_elems, flags, out):
        hists = self.torch.empty((elem_bytes, NSYM), dtype=self.torch.int64, device=self.device) if out is None else out
        self._call(name, d_in.data_ptr(), *base, _n_elems(d_in, elem_bytes, n_elems), elem_bytes, flags, hists.data_ptr())
        return hists

    def _compress_planes_out(self, d_in, elem_bytes, slots, n_elems, d_out, slot_bytes, d_codes, out_bytes=None):
        """the outputs of a planes compress call over `slots` slots, each allocated unless given -> its result dict"""
        t = self.torch
        n_elems = _n_elems(d_in, elem_bytes, n_elems)
        if slot_bytes is None:
            slot_bytes = planes_slot_bytes(n_elems)
        if d_out is None:
            d_out = self.empty_u8(slot_bytes * slots)
        if d_codes is None:
            d_codes = t.zeros((slots, C.sizeof(Code)), dtype=t.uint8, device=self.device)
        if out_bytes is None:
            out_bytes = t.zeros(slots, dtype=t.int64, device=self.device)
        return {"out": d_out, "slot_bytes": slot_bytes, "out_bytes": out_bytes, "codes": d_codes, "n_elems": n_elems,
                "elem_bytes": elem_bytes}

    def _compress_planes_coded(self, name, d_in, base, elem_bytes, d_codes, flags, n_elems, d_out, slot_bytes, indexes):
        if flags is None:
            flags = PLANES_BUILD_CODES if d_codes is None else 0
        r = self._compress_planes_out(d_in, elem_bytes, elem_bytes, n_elems, d_out, slot_bytes, d_codes)
        self._call(name, d_in.data_ptr(), *base, r["n_elems"], elem_bytes, r["codes"].data_ptr(), flags, r["out"].data_ptr(),
                   r["slot_bytes"], r["out_bytes"].data_ptr(), indexes)
        return r

    def _range_out(self, d_out, n_bytes, cap):
        """(d_out, cap) of a decode: d_out of n_bytes unless given, cap all of d_out unless given"""
        if d_out is None:
            d_out = self.empty_u8(n_bytes)
        return d_out, d_out.numel() if cap is None else cap

    def _decode_planes(self, name, streams, stream_bytes, slots, d_codes, indexes, more, n_elems, elem_bytes, d_out, cap, nbytes):
        """the whole-tensor plane decodes over `slots` streams; `more`: what the entry point takes between the side-cars and
        n_elems.  -> (d_out uint8, nbytes int64[1] device)"""
        d_out, cap = self._range_out(d_out, n_elems * elem_bytes, cap)
        if nbytes is None:
            nbytes = self.torch.zeros(1, dtype=self.torch.int64, device=self.device)
        self._call(name, _ptr_array(streams, slots), _size_array(stream_bytes, slots), _addr(d_codes), indexes, *more, n_elems,
                   elem_bytes, d_out.data_ptr(), cap, nbytes.data_ptr())
        return d_out, nbytes

    def _decode_planes_range(self, name, streams, stream_bytes, slots, d_codes, indexes, infos, d_tables, table_bytes, more, elem_bytes,
                             first, count, d_out, cap):
        """the range plane decodes over `slots` streams; `more`: what the entry point takes between the seek tables and
        elem_bytes.  -> d_out"""
        d_out, cap = self._range_out(d_out, count * elem_bytes, cap)
        self._call(name, _ptr_array(streams, slots), _size_array(stream_bytes, slots), _addr(d_codes), indexes,
                   *_seek_tables(infos, d_tables, table_bytes, slots), *more, elem_bytes, first, count, d_out.data_ptr(), cap)
        return d_out

    def _decode_planes_ranked_range(self, name, streams, stream_bytes, d_codes, ranks, more, n_elems, elem_bytes, first, count, indexes,
                                    infos, d_tables, table_bytes, d_out, cap):
        """the range decodes of 2 * elem_bytes slots with rank tables in HOST memory; `more`: what the entry point takes between
        the rank tables and n_elems"""
        r_infos, r_ptrs, _, keep = _rank_arrays(ranks, elem_bytes, device=False)
        d_out = self._decode_planes_range(name, streams, stream_bytes, 2 * elem_bytes, d_codes, indexes, infos, d_tables, table_bytes,
                                          (r_infos, r_ptrs) + more + (n_elems,), elem_bytes, first, count, d_out, cap)
        del keep  # the tables r_ptrs points into had to live until here
        return d_out

    def _decode_planes_gather(self, name, streams, stream_bytes, slots, d_codes, infos, d_tables, table_bytes, more, n_elems, elem_bytes,
                              d_index, row_elems, index_stride, n_rows, d_out, out_stride, d_row_status):
        """the row gathers over `slots` streams; `more`: what the entry point takes between the seek tables and n_elems.
        -> (d_out, d_row_status)"""
        t = self.torch
        n_rows = d_index.numel() if n_rows is None else n_rows
        index_stride = row_elems if index_stride is None else index_stride
        out_stride = row_elems * elem_bytes if out_stride is None else out_stride
        if d_out is None:
            d_out = self.empty_u8(max(n_rows, 1) * out_stride)
        if d_row_status is None:
            d_row_status = t.zeros(max(n_rows, 1), dtype=t.int32, device=self.device)
        self._call(name, _ptr_array(streams, slots), _size_array(stream_bytes, slots), _addr(d_codes),
                   *_seek_tables(infos, d_tables, table_bytes, slots), *more, n_elems, elem_bytes, d_index.data_ptr(), index_stride,
                   row_elems, n_rows, d_out.data_ptr(), out_stride, d_row_status.data_ptr())
        return d_out, d_row_status

    def planes_split(self, d_in, elem_bytes, n_elems=None, d_planes=None, plane_stride=None):
        """byte b of element k of d_in -> d_planes[b * plane_stride + k].  -> (d_planes uint8, plane_stride)"""
        return self._planes_split("ghf_planes_split", d_in, (), elem_bytes, n_elems, d_planes, plane_stride)

    def planes_merge(self, d_planes, plane_stride, n_elems, elem_bytes, d_out=None):
        """the inverse of planes_split.  -> d_out uint8[n_elems * elem_bytes]"""
        return self._planes_merge("ghf_planes_merge", d_planes, plane_stride, (), (n_elems,), n_elems, elem_bytes, d_out)

    def planes_index_alloc(self, n_elems, elem_bytes):
        """elem_bytes side-cars of n_elems symbols as the ctypes array compress_planes / decode_planes take"""
        arr = (Index * elem_bytes)()
        for p in range(elem_bytes):
            self._chk(self.L.ghf_index_alloc(self.h, n_elems, C.byref(arr[p])), "ghf_index_alloc")
        return arr

    def planes_index_free(self, arr):
        for ix in arr:
            self.L.ghf_index_free(self.h, C.byref(ix))

    def compress_planes(self, d_in, elem_bytes, n_elems=None, d_out=None, slot_bytes=None, d_codes=None, indexes=None):
        """d_in: a CUDA tensor of elements (any dtype; elem_bytes says how wide an element is).  Plane p's .crs2 image goes to
        d_out[p * slot_bytes ..); no host synchronisation.  indexes: None or planes_index_alloc(n_elems, elem_bytes).
        -> dict(out, slot_bytes, out_bytes int64[elem_bytes], codes uint8[elem_bytes, sizeof(Code)], n_elems, elem_bytes)"""
        r = self._compress_planes_out(d_in, elem_bytes, elem_bytes, n_elems, d_out, slot_bytes, d_codes)
        self._call("ghf_compress_planes", d_in.data_ptr(), r["n_elems"], elem_bytes, r["out"].data_ptr(), r["slot_bytes"],
                   r["out_bytes"].data_ptr(), r["codes"].data_ptr(), indexes)
        return r

    def histogram_planes(self, d_in, elem_bytes, n_elems=None, flags=0, out=None):
        """the byte counts of every byte plane of one tensor, in one pass: an int64[elem_bytes, 257] CUDA tensor, ready for
        build_codes.  flags: HIST_COVER_ALL.  No host synchronisation."""
        return self._histogram_planes("ghf_histogram_planes", d_in, (), elem_bytes, n_elems, flags, out)

    def planes_image_bytes(self, d_hists, d_codes, elem_bytes, out=None):
        """what planes with the counts d_hists (int64[elem_bytes, 257]) compress to under d_codes: int64[elem_bytes], 0 for
        a plane whose code is not complete or misses a counted byte.  No host synchronisation."""
        nbytes = self.torch.zeros(elem_bytes, dtype=self.torch.int64, device=self.device) if out is None else out
        self._chk(self.L.ghf_planes_image_bytes(self.h, d_hists.data_ptr(), d_codes.data_ptr(), elem_bytes, nbytes.data_ptr()),
                  "ghf_planes_image_bytes")
        return nbytes

    def compress_planes_coded(self, d_in, elem_bytes, d_codes=None, flags=None, n_elems=None, d_out=None, slot_bytes=None,
                              indexes=None):
        """compress_planes with one histogram pass and the codes either built in one launch (d_codes None or flags
        PLANES_BUILD_CODES: they are returned) or brought by the caller (d_codes uint8[elem_bytes, sizeof(Code)], flags 0).
        No host synchronisation.  -> the dict of compress_planes"""
        return self._compress_planes_coded("ghf_compress_planes_coded", d_in, (), elem_bytes, d_codes, flags, n_elems, d_out, slot_bytes,
                                           indexes)

    def decode_planes(self, streams, stream_bytes, d_codes, n_elems, elem_bytes, indexes=None, d_out=None, cap=None, nbytes=None):
        """streams: elem_bytes CUDA uint8 tensors (e.g. the slots of compress_planes), stream_bytes: their sizes as host
        ints.  indexes=None: the side-car-less path (synchronises).  -> (d_out uint8, nbytes int64[1] device)"""
        return self._decode_planes("ghf_decode_planes", streams, stream_bytes, elem_bytes, d_codes, indexes, (), n_elems, elem_bytes,
                                   d_out, cap, nbytes)

    def planes_merge_range(self, d_planes, plane_stride, first, count, elem_bytes, d_out=None):
        """elements [first, first + count) of the planes, interleaved.  -> d_out uint8[count * elem_bytes]"""
        return self._planes_merge("ghf_planes_merge_range", d_planes, plane_stride, (), (first, count), count, elem_bytes, d_out)

    def decode_planes_range(self, streams, stream_bytes, d_codes, elem_bytes, first, count, indexes=None, infos=None,
                            d_tables=None, table_bytes=None, d_out=None, cap=None):
        """d_out[0 .. count * elem_bytes) = elements [first, first + count) of the planes' decoded elements.  streams,
        stream_bytes, d_codes as for decode_planes; give either indexes (planes_index_alloc) or infos (elem_bytes SeekInfo)
        with d_tables (elem_bytes CUDA uint8 tensors).  Never synchronises.  -> d_out uint8"""
        return self._decode_planes_range("ghf_decode_planes_range", streams, stream_bytes, elem_bytes, d_codes, indexes, infos, d_tables,
                                         table_bytes, (), elem_bytes, first, count, d_out, cap)

    # ---- byte planes against a base tensor: the calls above on d_in ^ d_base, the XOR inside their
    # streaming kernels.  d_base: a CUDA tensor of the same bytes as d_in / d_out (the range calls: of the range's own
    # elements); it may be d_out itself in the merging calls ----------------------------------------------------------
    def histogram_planes_delta(self, d_in, d_base, elem_bytes, n_elems=None, flags=0, out=None):
        """histogram_planes of d_in ^ d_base in one pass over both; nothing is materialised.  -> int64[elem_bytes, 257]"""
        return self._histogram_planes("ghf_histogram_planes_delta", d_in, (_addr(d_base),), elem_bytes, n_elems, flags, out)

    def planes_split_delta(self, d_in, d_base, elem_bytes, n_elems=None, d_planes=None, plane_stride=None):
        """planes_split of d_in ^ d_base.  -> (d_planes uint8, plane_stride)"""
        return self._planes_split("ghf_planes_split_delta", d_in, (_addr(d_base),), elem_bytes, n_elems, d_planes, plane_stride)

    def planes_merge_delta(self, d_planes, plane_stride, d_base, n_elems, elem_bytes, d_out=None):
        """d_out = planes_merge(d_planes) ^ d_base; d_out may be d_base.  -> d_out uint8[n_elems * elem_bytes]"""
        return self._planes_merge("ghf_planes_merge_delta", d_planes, plane_stride, (_addr(d_base),), (n_elems,), n_elems, elem_bytes,
                                  d_out)

    def planes_merge_range_delta(self, d_planes, plane_stride, d_base, first, count, elem_bytes, d_out=None):
        """planes_merge_range ^ d_base, where d_base holds base elements [first, first + count) and is indexed like d_out
        (and may be d_out).  -> d_out uint8[count * elem_bytes]"""
        return self._planes_merge("ghf_planes_merge_range_delta", d_planes, plane_stride, (_addr(d_base),), (first, count), count,
                                  elem_bytes, d_out)

    def compress_planes_delta(self, d_in, d_base, elem_bytes, d_codes=None, flags=None, n_elems=None, d_out=None, slot_bytes=None,
                              indexes=None):
        """compress_planes_coded of d_in ^ d_base: every image is an ordinary .crs2 of a plane of the XOR.  No host
        synchronisation.  -> the dict of compress_planes"""
        return self._compress_planes_coded("ghf_compress_planes_delta", d_in, (_addr(d_base),), elem_bytes, d_codes, flags, n_elems,
                                           d_out, slot_bytes, indexes)

    def decode_planes_delta(self, streams, stream_bytes, d_codes, d_base, n_elems, elem_bytes, indexes=None, d_out=None, cap=None,
                            nbytes=None):
        """decode_planes, then ^ d_base in the merge; d_out may be d_base (behind a latched status it then still holds the
        base).  indexes=None synchronises.  -> (d_out uint8, nbytes int64[1] device)"""
        return self._decode_planes("ghf_decode_planes_delta", streams, stream_bytes, elem_bytes, d_codes, indexes, (_addr(d_base),),
                                   n_elems, elem_bytes, d_out, cap, nbytes)

    def decode_planes_range_delta(self, streams, stream_bytes, d_codes, d_base, elem_bytes, first, count, indexes=None, infos=None,
                                  d_tables=None, table_bytes=None, d_out=None, cap=None):
        """decode_planes_range, then ^ d_base in the merge: d_base holds base elements [first, first + count), indexed like
        d_out, and may be d_out.  Never synchronises.  -> d_out uint8"""
        return self._decode_planes_range("ghf_decode_planes_range_delta", streams, stream_bytes, elem_bytes, d_codes, indexes, infos,
                                         d_tables, table_bytes, (_addr(d_base),), elem_bytes, first, count, d_out, cap)

    # ---- zero-suppressed byte planes: a byte string as a bit mask of its non-zero bytes plus those
    # bytes; planes that are almost all zeros stored as two ordinary .crs2 images, mask and values -------------------------
    sparse_mask_bytes = staticmethod(sparse_mask_bytes)

    def sparse_split(self, d_in, n=None, d_mask=None, d_vals=None, vals_cap=None, n_vals=None):
        """d_in uint8[n] -> (d_mask uint8[(n + 7) // 8], d_vals uint8, n_vals int64[1] device).  No host synchronisation.
        More than vals_cap (default: d_vals.numel(), or n) non-zero bytes latch GHF_E_CAP: d_vals is then untouched, the mask
        and n_vals are written."""
        t = self.torch
        n = d_in.numel() if n is None else n
        if d_mask is None:
            d_mask = self.empty_u8(sparse_mask_bytes(n))
        if d_vals is None:
            d_vals = self.empty_u8(n if vals_cap is None else max(vals_cap, 1))
        if vals_cap is None:
            vals_cap = d_vals.numel()
        if n_vals is None:
            n_vals = t.zeros(1, dtype=t.int64, device=self.device)
        self._chk(self.L.ghf_sparse_split(self.h, d_in.data_ptr(), n, d_mask.data_ptr(), d_vals.data_ptr(), vals_cap, n_vals.data_ptr()),
                  "ghf_sparse_split")
        return d_mask, d_vals, n_vals

    def sparse_merge(self, d_mask, d_vals, n_vals, n, d_out=None):
        """the inverse of sparse_split (n_vals: a host int; d_vals may be None when it is 0).  -> d_out uint8[n].  A mask whose
        set bits do not number n_vals, or with a set pad bit, latches GHF_E_CORRUPT and nothing is stored."""
        if d_out is None:
            d_out = self.empty_u8(n)
        self._chk(self.L.ghf_sparse_merge(self.h, d_mask.data_ptr(), None if d_vals is None else d_vals.data_ptr(), n_vals, n,
                                          d_out.data_ptr()), "ghf_sparse_merge")
        return d_out

    def _rank_slots(self, n_elems, elem_bytes, d_ranks, rank_slot_bytes, alloc):
        """(d_ranks, rank_slot_bytes): a slot is by default the rank table of n_elems bytes rounded up to 16; elem_bytes of
        them are allocated when `alloc` says so and none are given"""
        if rank_slot_bytes is None:
            rank_slot_bytes = (sparse_rank_bytes(n_elems) + 15) & ~15
        if d_ranks is None and alloc:
            d_ranks = self.empty_u8(rank_slot_bytes * elem_bytes)
        return d_ranks, rank_slot_bytes

    def _compress_planes_sparse(self, name, d_in, base, elem_bytes, sparse_planes, n_elems, d_out, slot_bytes, d_codes, indexes,
                                ranks=None):
        """the four sparse compress calls; ranks: None, or (d_ranks, rank_slot_bytes) of the two that write rank tables"""
        r = self._compress_planes_out(d_in, elem_bytes, 2 * elem_bytes, n_elems, d_out, slot_bytes, d_codes)
        idx = (Index * (2 * elem_bytes))() if indexes else None
        chosen, n_vals = C.c_uint(0), (C.c_size_t * elem_bytes)()
        tail = ()
        if ranks is not None:
            d_ranks, rank_slot_bytes = self._rank_slots(r["n_elems"], elem_bytes, *ranks, alloc=True)
            tail = (d_ranks.data_ptr(), rank_slot_bytes)
        self._call(name, d_in.data_ptr(), *base, r["n_elems"], elem_bytes, sparse_planes, r["out"].data_ptr(), r["slot_bytes"],
                   r["out_bytes"].data_ptr(), r["codes"].data_ptr(), idx, C.byref(chosen), n_vals, *tail)
        r.update(sparse_planes=int(chosen.value), n_vals=[int(v) for v in n_vals], indexes=idx)
        if ranks is not None:
            r.update(ranks=d_ranks, rank_slot_bytes=rank_slot_bytes)
        return r

    def compress_planes_sparse(self, d_in, elem_bytes, sparse_planes=SPARSE_AUTO, n_elems=None, d_out=None, slot_bytes=None,
                               d_codes=None, indexes=False):
        """the byte planes of d_in, the planes in sparse_planes (a bit per plane, or SPARSE_AUTO: at least 3/4 zero bytes) stored
        as mask + values: 2 * elem_bytes slots, slot p = plane p or its mask, slot elem_bytes + p = its values or empty.
        SYNCHRONISES once (the plane counts).  indexes=True: the call allocates a side-car per stored stream (free them with
        planes_index_free).  -> the dict of compress_planes over 2 * elem_bytes slots, plus sparse_planes (the planes stored
        sparse), n_vals (host ints, per plane) and indexes (a ctypes Index array or None)"""
        return self._compress_planes_sparse("ghf_compress_planes_sparse", d_in, (), elem_bytes, sparse_planes, n_elems, d_out, slot_bytes,
                                            d_codes, indexes)

    def compress_planes_sparse_delta(self, d_in, d_base, elem_bytes, sparse_planes=SPARSE_AUTO, n_elems=None, d_out=None,
                                     slot_bytes=None, d_codes=None, indexes=False):
        """compress_planes_sparse of d_in ^ d_base (the XOR inside the histogram and split kernels).  -> the same dict"""
        return self._compress_planes_sparse("ghf_compress_planes_sparse_delta", d_in, (_addr(d_base),), elem_bytes, sparse_planes, n_elems,
                                            d_out, slot_bytes, d_codes, indexes)

    def decode_planes_sparse(self, streams, stream_bytes, d_codes, sparse_planes, n_vals, n_elems, elem_bytes, indexes=None,
                             d_out=None, cap=None, nbytes=None):
        """streams: 2 * elem_bytes CUDA uint8 tensors (None for an empty slot), stream_bytes: their sizes as host ints;
        sparse_planes and n_vals as compress_planes_sparse returned them.  indexes=None synchronises per stream.
        -> (d_out uint8, nbytes int64[1] device)"""
        return self._decode_planes("ghf_decode_planes_sparse", streams, stream_bytes, 2 * elem_bytes, d_codes, indexes,
                                   (sparse_planes, _size_array(n_vals, elem_bytes)), n_elems, elem_bytes, d_out, cap, nbytes)

    def decode_planes_sparse_delta(self, streams, stream_bytes, d_codes, d_base, sparse_planes, n_vals, n_elems, elem_bytes,
                                   indexes=None, d_out=None, cap=None, nbytes=None):
        """decode_planes_sparse, then ^ d_base in the merge; d_out may be d_base (behind a latched status it then still holds
        the base).  -> (d_out uint8, nbytes int64[1] device)"""
        return self._decode_planes("ghf_decode_planes_sparse_delta", streams, stream_bytes, 2 * elem_bytes, d_codes, indexes,
                                   (_addr(d_base), sparse_planes, _size_array(n_vals, elem_bytes)), n_elems, elem_bytes, d_out, cap, nbytes)

    # ---- an element range of zero-suppressed byte planes: rank tables, the merge with values that start
    # anywhere, the compress calls that write rank tables, the range decode -------------------------------------------------
    sparse_rank_bytes = staticmethod(sparse_rank_bytes)
    sparse_rank_parse = staticmethod(sparse_rank_parse)

    def sparse_rank_pack(self, d_mask, n, d_table=None, cap=None):
        """mask (device) of a byte string of n bytes -> its rank table image in device memory.  No host synchronisation."""
        if d_table is None:
            d_table = self.empty_u8(sparse_rank_bytes(n))
        self._chk(self.L.ghf_sparse_rank_pack(self.h, d_mask.data_ptr(), n, d_table.data_ptr(), d_table.numel() if cap is None else cap),
                  "ghf_sparse_rank_pack")
        return d_table

    def sparse_merge_at(self, d_mask, d_vals, vals_skip, n_vals, n, d_out=None):
        """sparse_merge with the values at d_vals[vals_skip : vals_skip + n_vals] (d_vals itself 16-byte aligned).  -> d_out"""
        if d_out is None:
            d_out = self.empty_u8(n)
        self._chk(self.L.ghf_sparse_merge_at(self.h, d_mask.data_ptr(), None if d_vals is None else d_vals.data_ptr(), vals_skip, n_vals, n,
                                             d_out.data_ptr()), "ghf_sparse_merge_at")
        return d_out

    def compress_planes_sparse_ranked(self, d_in, elem_bytes, sparse_planes=SPARSE_AUTO, n_elems=None, d_out=None, slot_bytes=None,
                                      d_codes=None, indexes=False, d_ranks=None, rank_slot_bytes=None):
        """compress_planes_sparse, and the rank table of every sparse plane in slot p of `ranks` (device uint8, elem_bytes slots
        of rank_slot_bytes; slots of dense planes stay unwritten).  -> the same dict plus ranks and rank_slot_bytes"""
        return self._compress_planes_sparse("ghf_compress_planes_sparse_ranked", d_in, (), elem_bytes, sparse_planes, n_elems, d_out,
                                            slot_bytes, d_codes, indexes, ranks=(d_ranks, rank_slot_bytes))

    def compress_planes_sparse_ranked_delta(self, d_in, d_base, elem_bytes, sparse_planes=SPARSE_AUTO, n_elems=None, d_out=None,
                                            slot_bytes=None, d_codes=None, indexes=False, d_ranks=None, rank_slot_bytes=None):
        """compress_planes_sparse_ranked of d_in ^ d_base.  -> the same dict"""
        return self._compress_planes_sparse("ghf_compress_planes_sparse_ranked_delta", d_in, (_addr(d_base),), elem_bytes, sparse_planes,
                                            n_elems, d_out, slot_bytes, d_codes, indexes, ranks=(d_ranks, rank_slot_bytes))

    def decode_planes_sparse_range(self, streams, stream_bytes, d_codes, sparse_planes, ranks, n_elems, elem_bytes, first, count,
                                   indexes=None, infos=None, d_tables=None, table_bytes=None, d_out=None, cap=None):
        """d_out[0 : count * elem_bytes] = elements [first, first + count) of a tensor stored by compress_planes_sparse[_ranked].
        streams / stream_bytes / infos / d_tables: 2 * elem_bytes entries (None for an empty slot); ranks: per plane None or
        (SparseRankInfo, the table as HOST bytes); give either indexes or (infos, d_tables).  Never synchronises.  -> d_out"""
        return self._decode_planes_ranked_range("ghf_decode_planes_sparse_range", streams, stream_bytes, d_codes, ranks, (sparse_planes,),
                                                n_elems, elem_bytes, first, count, indexes, infos, d_tables, table_bytes, d_out, cap)

    def decode_planes_sparse_range_delta(self, streams, stream_bytes, d_codes, d_base, sparse_planes, ranks, n_elems, elem_bytes, first,
                                         count, indexes=None, infos=None, d_tables=None, table_bytes=None, d_out=None, cap=None):
        """decode_planes_sparse_range, then ^ d_base in the merge: d_base holds base elements [first, first + count), indexed like
        d_out, and may be d_out.  -> d_out"""
        return self._decode_planes_ranked_range("ghf_decode_planes_sparse_range_delta", streams, stream_bytes, d_codes, ranks,
                                                (_addr(d_base), sparse_planes), n_elems, elem_bytes, first, count, indexes, infos,
                                                d_tables, table_bytes, d_out, cap)

    # ---- byte planes in three forms: raw planes beside dense and sparse ones; d_base is optional ------
    _plane_ptrs = staticmethod(_ptr_array)  # (planes, elem_bytes): CUDA uint8 tensors or raw device addresses -> a host array

    def planes_split_to(self, d_in, planes, elem_bytes, n_elems=None, d_base=None):
        """plane p of d_in (of d_in ^ d_base) -> planes[p][0 : n_elems]; planes: elem_bytes CUDA uint8 tensors (or device
        addresses), each 16-byte aligned, anywhere and in any order.  No host synchronisation.  -> planes"""
        self._call("ghf_planes_split_to", d_in.data_ptr(), _addr(d_base), _n_elems(d_in, elem_bytes, n_elems), elem_bytes,
                   _ptr_array(planes, elem_bytes))
        return planes

    def planes_merge_from(self, planes, n_elems, elem_bytes, d_out=None, d_base=None):
        """the inverse of planes_split_to; d_out may be d_base.  -> d_out uint8[n_elems * elem_bytes]"""
        if d_out is None:
            d_out = self.empty_u8(n_elems * elem_bytes)
        self._call("ghf_planes_merge_from", _ptr_array(planes, elem_bytes), _addr(d_base), n_elems, elem_bytes, d_out.data_ptr())
        return d_out

    def planes_merge_range_from(self, planes, count, elem_bytes, d_out=None, d_base=None):
        """planes[p]: the address (or a tensor view that starts there) of plane p's byte of the run's first element; all equal
        modulo 16.  d_base: the base elements of the run, indexed like d_out.  -> d_out uint8[count * elem_bytes]"""
        if d_out is None:
            d_out = self.empty_u8(count * elem_bytes)
        self._call("ghf_planes_merge_range_from", _ptr_array(planes, elem_bytes), _addr(d_base), count, elem_bytes, d_out.data_ptr())
        return d_out

    def compress_planes_forms(self, d_in, elem_bytes, raw_planes=RAW_AUTO, sparse_planes=0, d_base=None, n_elems=None, d_out=None,
                              slot_bytes=None, d_codes=None, indexes=False, ranks=False, d_ranks=None, rank_slot_bytes=None,
                              out_bytes=None):
        """the byte planes of d_in (of d_in ^ d_base), each stored raw, sparse or dense: raw_planes / sparse_planes are a bit
        per plane, or RAW_AUTO (raw exactly when the plane's image would be at least n_elems bytes) / SPARSE_AUTO.  A raw plane
        is its n_elems bytes at the start of slot p, written by the split itself.  SYNCHRONISES at most once; never with both
        masks explicit and sparse_planes == 0.  ranks=True (or d_ranks): the rank table of every sparse plane.
        -> the dict of compress_planes_sparse_ranked plus raw_planes (the planes stored raw)"""
        r = self._compress_planes_out(d_in, elem_bytes, 2 * elem_bytes, n_elems, d_out, slot_bytes, d_codes, out_bytes)
        d_ranks, rank_slot_bytes = self._rank_slots(r["n_elems"], elem_bytes, d_ranks, rank_slot_bytes, alloc=ranks)
        idx = (Index * (2 * elem_bytes))() if indexes else None
        raw, chosen, n_vals = C.c_uint(0), C.c_uint(0), (C.c_size_t * elem_bytes)()
        self._call("ghf_compress_planes_forms", d_in.data_ptr(), _addr(d_base), r["n_elems"], elem_bytes, raw_planes, sparse_planes,
                   r["out"].data_ptr(), r["slot_bytes"], r["out_bytes"].data_ptr(), r["codes"].data_ptr(), idx, _addr(d_ranks),
                   rank_slot_bytes, C.byref(raw), C.byref(chosen), n_vals)
        r.update(raw_planes=int(raw.value), sparse_planes=int(chosen.value), n_vals=[int(v) for v in n_vals], indexes=idx, ranks=d_ranks,
                 rank_slot_bytes=rank_slot_bytes)
        return r

    def decode_planes_forms(self, streams, stream_bytes, d_codes, raw_planes, sparse_planes, n_vals, n_elems, elem_bytes, indexes=None,
                            d_base=None, d_out=None, cap=None, nbytes=None):
        """streams: 2 * elem_bytes CUDA uint8 tensors (None for an empty slot; a raw plane's holds the plane itself and its
        stream_bytes entry is n_elems); raw_planes, sparse_planes and n_vals as compress_planes_forms returned them.  A raw
        plane is read where it lies.  d_out may be d_base.  indexes=None synchronises per stream that has a code.
        -> (d_out uint8, nbytes int64[1] device)"""
        return self._decode_planes("ghf_decode_planes_forms", streams, stream_bytes, 2 * elem_bytes, d_codes, indexes,
                                   (_addr(d_base), raw_planes, sparse_planes, _size_array(n_vals, elem_bytes)), n_elems, elem_bytes, d_out,
                                   cap, nbytes)

    def decode_planes_forms_range(self, streams, stream_bytes, d_codes, raw_planes, sparse_planes, ranks, n_elems, elem_bytes, first,
                                  count, indexes=None, infos=None, d_tables=None, table_bytes=None, d_base=None, d_out=None, cap=None):
        """d_out[0 : count * elem_bytes] = elements [first, first + count) of a tensor stored by compress_planes_forms; the
        arguments of decode_planes_sparse_range plus raw_planes and the optional d_base (the base elements of the range, indexed
        like d_out).  The index, info and table entries of a raw plane may be None.  Never synchronises.  -> d_out"""
        return self._decode_planes_ranked_range("ghf_decode_planes_forms_range", streams, stream_bytes, d_codes, ranks,
                                                (_addr(d_base), raw_planes, sparse_planes), n_elems, elem_bytes, first, count, indexes,
                                                infos, d_tables, table_bytes, d_out, cap)

    def decode_planes_gather(self, streams, stream_bytes, d_codes, raw_planes, n_elems, elem_bytes, d_index, row_elems, index_stride=None,
                             infos=None, d_tables=None, table_bytes=None, n_rows=None, d_out=None, out_stride=None, d_row_status=None):
        """rows [d_index[r] * index_stride, + row_elems) of a tensor stored by compress_planes_forms without sparse planes, ONE
        launch whatever the number of rows: streams / stream_bytes / infos / d_tables are the first elem_bytes entries of
        decode_planes_forms_range's (seek tables are the only source of run starts; a raw plane's info and table may be None).
        d_index: int64 / uint64 CUDA tensor of row indices; index_stride defaults to row_elems (a lookup by row id).  d_out
        (uint8, out_stride bytes from row to row, default row_elems * elem_bytes) and d_row_status (int32[n_rows]) are
        allocated when not given.  A failed row stores nothing and never latches the context.  Never synchronises.
        -> (d_out, d_row_status)"""
        return self._decode_planes_gather("ghf_decode_planes_gather", streams, stream_bytes, elem_bytes, d_codes, infos, d_tables,
                                          table_bytes, (raw_planes,), n_elems, elem_bytes, d_index, row_elems, index_stride, n_rows, d_out,
                                          out_stride, d_row_status)

    def decode_planes_gather_forms(self, streams, stream_bytes, d_codes, raw_planes, sparse_planes, ranks, n_elems, elem_bytes, d_index,
                                   row_elems, index_stride=None, infos=None, d_tables=None, table_bytes=None, d_base=None, n_rows=None,
                                   d_out=None, out_stride=None, d_row_status=None):
        """decode_planes_gather for a tensor stored by compress_planes_forms in any mix of the three forms, against the WHOLE base
        tensor d_base where there is one: ONE launch whatever the number of rows.  streams / stream_bytes / infos / d_tables
        have 2 * elem_bytes entries, indexed like decode_planes_forms_range's (None for a slot that is not stored).  ranks: per
        plane None, or (SparseRankInfo, the rank table as a CUDA uint8 tensor of sparse_rank_bytes(n_elems)) for a sparse
        plane -- the image lies in DEVICE memory here.  The row cap is GATHER_SPARSE_MAX_ROW_ELEMS with a sparse plane.
        Never synchronises.  -> (d_out, d_row_status)"""
        r_infos, r_ptrs, r_bytes, _ = _rank_arrays(ranks, elem_bytes, device=True)
        return self._decode_planes_gather("ghf_decode_planes_gather_forms", streams, stream_bytes, 2 * elem_bytes, d_codes, infos, d_tables,
                                          table_bytes, (r_infos, r_ptrs, r_bytes, _addr(d_base), raw_planes, sparse_planes), n_elems,
                                          elem_bytes, d_index, row_elems, index_stride, n_rows, d_out, out_stride, d_row_status)

    # ---- seekable streams: the seek table (the persistent form of the side-car) ----------------
    def seek_pack(self, index, d_stream=None, stream_bytes=0, d_table=None, n=None):
        """side-car -> table image in device memory (a uint8 tensor of seek_bytes(n_symbols)).  index=None: the side-car
        decoded_size() last rebuilt for (d_stream, stream_bytes); n = what decoded_size() returned."""
        if d_table is None:
            d_table = self.torch.empty(seek_bytes(index.n_symbols if index is not None else n), dtype=self.torch.uint8,
                                       device=self.device)
        self._chk(self.L.ghf_seek_pack(self.h, None if index is None else C.byref(index),
                                       None if d_stream is None else d_stream.data_ptr(), stream_bytes, d_table.data_ptr(),
                                       d_table.numel()), "ghf_seek_pack")
        return d_table

    def seek_expand(self, info, d_table, d_stream, stream_bytes, d_code, index=None, table_bytes=None):
        """table (device) -> full side-car; -> the index (allocated here unless given)"""
        if index is None:
            index = self.index_alloc(info.n_symbols)
        tb = seek_bytes(info.n_symbols) if table_bytes is None else table_bytes
        self._chk(self.L.ghf_seek_expand(self.h, C.byref(info), d_table.data_ptr(), tb, d_stream.data_ptr(), stream_bytes,
                                         d_code.data_ptr(), C.byref(index)), "ghf_seek_expand")
        return index

    def decode_range(self, d_stream, stream_bytes, d_code, first, count, index=None, info=None, d_table=None, d_out=None,
                     cap=None, table_bytes=None):
        """d_out[0..count) = decoded bytes [first, first + count); give either index or (info, d_table)"""
        if d_out is None:
            d_out = self.empty_u8(count)
        if table_bytes is None:
            table_bytes = seek_bytes(info.n_symbols) if info is not None else 0
        self._chk(
            self.L.ghf_decode_range(self.h, d_stream.data_ptr(), stream_bytes, d_code.data_ptr(),
                                    None if index is None else C.byref(index), None if info is None else C.byref(info),
                                    None if d_table is None else d_table.data_ptr(), table_bytes, first, count,
                                    d_out.data_ptr(), d_out.numel() if cap is None else cap),
            "ghf_decode_range")
        return d_out

    def sync_piece(self, d_piece, piece_bytes, first_bit, end_bit, d_code):
        """one rank's piece of a side-car-less stream (multi-GPU decode): -> (landing, n_symbols, has_end_mark)"""
        landing, n, eof = C.c_uint64(0), C.c_uint64(0), C.c_int(0)
        self._chk(self.L.ghf_sync_piece(self.h, d_piece.data_ptr(), piece_bytes, first_bit, end_bit, d_code.data_ptr(),
                                        C.byref(landing), C.byref(n), C.byref(eof)), "ghf_sync_piece")
        return landing.value, n.value, bool(eof.value)

    # ---- sharded streams over RCCL, C ABI ------------------------------------------
    def comm_init(self, unique_id, world, rank):
        """-> opaque ghf_comm handle (ncclCommInitRank on this context's device)"""
        h = C.c_void_p()
        self._chk(self.L.ghf_comm_init_rank(self.h, unique_id, world, rank, C.byref(h)), "ghf_comm_init_rank")
        return h

    def comm_destroy(self, comm):
        if comm:
            self.L.ghf_comm_destroy(comm)

    def comm_allreduce_hist(self, comm, d_hist):
        self._chk(self.L.ghf_comm_allreduce_hist(self.h, comm, d_hist.data_ptr()), "ghf_comm_allreduce_hist")

    def comm_allgather_total(self, comm, d_total, d_totals):
        self._chk(self.L.ghf_comm_allgather_total(self.h, comm, d_total.data_ptr(), d_totals.data_ptr()), "ghf_comm_allgather_total")

    def encode_sharded(self, comm, d_in, d_out=None, d_code=None, index=None, n=None):
        """ghf_encode_sharded: this rank's shard, collectives included, one call. -> dict like sharded.encode_sharded"""
        n = d_in.numel() if n is None else n
        if d_out is None:
            d_out = self.empty_u8(shard_bound(n))
        if d_code is None:
            d_code = self.new_code()
        start = self.torch.zeros(1, dtype=self.torch.int64, device=self.device)
        end = self.torch.zeros(2, dtype=self.torch.int64, device=self.device)
        self._chk(
            self.L.ghf_encode_sharded(self.h, comm, d_in.data_ptr(), n, d_out.data_ptr(), d_out.numel(), d_code.data_ptr(),
                                      None if index is None else C.byref(index), start.data_ptr(), end.data_ptr()),
            "ghf_encode_sharded")
        return {"out": d_out, "start_bit": start, "end": end, "code": d_code}

    # ---- .crs (NormalHuffEncoder / NormalHuffDecoder) ---------------------------
    def new_tree(self):
        return self.torch.zeros(C.sizeof(Tree), dtype=self.torch.uint8, device=self.device)

    def tree_to_host(self, d_tree):
        return Tree.from_buffer_copy(d_tree.cpu().numpy().tobytes())

    def tree_to_device(self, tree):
        import numpy as np

        return self.torch.from_numpy(np.frombuffer(bytes(tree), dtype=np.uint8).copy()).to(self.device)

    def crs_build_code(self, d_hist, d_tree=None, d_code=None):
        d_tree = self.new_tree() if d_tree is None else d_tree
        d_code = self.new_code() if d_code is None else d_code
        self._chk(self.L.ghf_crs_build_code(self.h, d_hist.data_ptr(), d_tree.data_ptr(), d_code.data_ptr()), "ghf_crs_build_code")
        return d_tree, d_code

    def crs_compress(self, d_in, d_out=None, d_tree=None, index=None, n=None):
        """-> (d_out, d_out_bytes[1] int64 device, d_tree)"""
        n = d_in.numel() if n is None else n
        if d_out is None:
            d_out = self.empty_u8(int(self.L.ghf_crs_compress_bound(n)))
        if d_tree is None:
            d_tree = self.new_tree()
        nbytes = self.torch.zeros(1, dtype=self.torch.int64, device=self.device)
        self._chk(
            self.L.ghf_crs_compress(self.h, d_in.data_ptr(), n, d_out.data_ptr(), d_out.numel(), nbytes.data_ptr(),
                                    d_tree.data_ptr(), None if index is None else C.byref(index)),
            "ghf_crs_compress")
        return d_out, nbytes, d_tree

    def crs_decoded_size(self, d_stream, stream_bytes, left_bits, d_tree):
        n = C.c_uint64(0)
        self._chk(self.L.ghf_crs_decoded_size(self.h, d_stream.data_ptr(), stream_bytes, left_bits, d_tree.data_ptr(), C.byref(n)),
                  "ghf_crs_decoded_size")
        return n.value

    def crs_sync_piece(self, d_piece, piece_bytes, first_bit, end_bit, d_tree):
        """one piece of a .crs body (no end mark in this format): -> (landing, n_symbols)"""
        landing, n = C.c_uint64(0), C.c_uint64(0)
        self._chk(self.L.ghf_crs_sync_piece(self.h, d_piece.data_ptr(), piece_bytes, first_bit, end_bit, d_tree.data_ptr(),
                                            C.byref(landing), C.byref(n)), "ghf_crs_sync_piece")
        return landing.value, n.value

    def crs_decode(self, d_stream, stream_bytes, left_bits, d_tree, index=None, d_out=None, cap=None, nbytes=None):
        """d_stream: the .crs image with the stored last byte appended behind the body when left_bits != 0."""
        if d_out is None:
            d_out = self.empty_u8(index.n_symbols if index is not None else cap)
        if nbytes is None:
            nbytes = self.torch.empty(1, dtype=self.torch.int64, device=self.device)
        self._chk(
            self.L.ghf_crs_decode(self.h, d_stream.data_ptr(), stream_bytes, left_bits, d_tree.data_ptr(),
                                  None if index is None else C.byref(index), d_out.data_ptr(), d_out.numel(), nbytes.data_ptr()),
            "ghf_crs_decode")
        return d_out, nbytes
