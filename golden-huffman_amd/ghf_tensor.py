"""ctypes binding of the container calls of lib/libghf.so (C ABI: include/ghf_tensor.h): one stored
object per typed tensor.  A module of its own beside ghf.py, with its own prototype table, bound on the handle ghf.lib()
returns; import it as golden_huffman_amd.ghf_tensor after pkgload.load().  Plumbing like ghf.py: device memory comes from torch
tensors, work is queued on the stream of the ghf.Context given, nothing is computed here."""
import ctypes as C

from . import ghf as _ghf

HEAD_BYTES = 768    # GHF_TENSOR_HEAD_BYTES: a container is opened from these
DIR_ENTRIES = 40    # GHF_TENSOR_DIR_ENTRIES: 16 streams, 16 seek tables, 8 rank tables
DELTA = 1           # GHF_TENSOR_DELTA: the planes are those of new ^ base
STREAMS, TABLES, RANKS = 0, 16, 32  # where the three groups begin in the directory


class Section(C.Structure):
    """ghf_tensor_section: {0, 0} is an absent section"""

    _fields_ = [("offset", C.c_uint64), ("bytes", C.c_uint64)]


class TensorInfo(C.Structure):
    """ghf_tensor_info: the head's fields and the 40 directory entries"""

    _fields_ = [("version", C.c_uint32), ("elem_bytes", C.c_uint32), ("n_elems", C.c_uint64), ("raw_planes", C.c_uint32),
                ("sparse_planes", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32), ("total_bytes", C.c_uint64),
                ("n_vals", C.c_uint64 * _ghf.PLANES_MAX), ("dir", Section * DIR_ENTRIES)]

    def sections(self):
        """the directory as a list of (offset, bytes)"""
        return [(int(s.offset), int(s.bytes)) for s in self.dir]


# ---- the prototypes, every exported function of include/ghf_tensor.h once: name -> (restype or None for int, argtypes)
_vp, _sz, _u64, _u32, _ui = C.c_void_p, C.c_size_t, C.c_uint64, C.c_uint32, C.c_uint
_pvp, _psz, _pidx, _pinfo = C.POINTER(_vp), C.POINTER(_sz), C.POINTER(_ghf.Index), C.POINTER(TensorInfo)
_PROTOS = {
    "ghf_tensor_bound": (_sz, [_sz, _u32]),
    "ghf_tensor_pack": (None, [_vp, _pvp, _vp, _pidx, _pvp, _ui, _ui, _psz, _sz, _u32, _ui, _vp, _sz, _vp]),
    "ghf_compress_tensor": (None, [_vp, _vp, _vp, _sz, _u32, _ui, _ui, _vp, _sz, _vp]),
    "ghf_tensor_workspace_release": (None, [_vp]),
    "ghf_tensor_parse": (None, [_vp, _sz, _sz, _pinfo]),
    "ghf_tensor_open": (None, [_vp, _vp, _sz, _vp, _sz, _pvp]),
    "ghf_tensor_close": (None, [_vp]),
    "ghf_tensor_describe": (None, [_vp, _pinfo]),
    "ghf_tensor_decode": (None, [_vp, _vp, _vp, _vp, _sz, _vp]),
    "ghf_tensor_decode_range": (None, [_vp, _vp, _vp, _u64, _u64, _vp, _sz]),
    "ghf_tensor_gather": (None, [_vp, _vp, _vp, _vp, _u64, _u32, _u32, _vp, _sz, _vp]),
}
EXPORTS = list(_PROTOS)

_bound = False


def lib():
    """the handle ghf.lib() returns, with this module's prototypes applied; raises when the library has not been built"""
    global _bound
    L = _ghf.lib()
    if not _bound:
        for name, (restype, argtypes) in _PROTOS.items():
            f = getattr(L, name)
            f.argtypes = argtypes
            if restype is not None:
                f.restype = restype
        _bound = True
    return L


def _addr(x):
    return None if x is None else x if isinstance(x, int) else x.data_ptr()


def _host(buf):
    """host bytes (numpy uint8, bytes) as a ctypes buffer the call may read"""
    raw = bytes(buf) if isinstance(buf, (bytes, bytearray)) else buf.tobytes()
    return (C.c_uint8 * max(len(raw), 1)).from_buffer_copy(raw.ljust(1, b"\0")), len(raw)


def bound(n_elems, elem_bytes):
    """a container capacity that suffices for any tensor of n_elems elements of elem_bytes bytes"""
    return int(lib().ghf_tensor_bound(n_elems, elem_bytes))


def parse(head, container_bytes=None):
    """ghf_tensor_parse of host bytes (at least HEAD_BYTES of them; container_bytes defaults to what the head states).
    -> TensorInfo; raises GhfError (status 6) for anything that is not the head of a container of that size"""
    buf, n = _host(head)
    if container_bytes is None:
        container_bytes = int.from_bytes(bytes(buf[40:48]), "little") if n >= 48 else 0
    info = TensorInfo()
    rc = lib().ghf_tensor_parse(buf, n, container_bytes, C.byref(info))
    if rc:
        raise _ghf.GhfError(rc, "ghf_tensor_parse")
    return info


def _container(ctx, n_elems, elem_bytes, d_container, cap, nbytes):
    t = ctx.torch
    if d_container is None:
        d_container = ctx.empty_u8(bound(n_elems, elem_bytes) if cap is None else cap)
    if nbytes is None:
        nbytes = t.zeros(1, dtype=t.int64, device=ctx.device)
    return d_container, d_container.numel() if cap is None else cap, nbytes


def compress_tensor(ctx, d_in, elem_bytes, raw_planes=_ghf.RAW_AUTO, sparse_planes=0, d_base=None, n_elems=None, d_container=None,
                    cap=None, nbytes=None):
    """d_in (against d_base where given: the head then carries DELTA) -> one container.  raw_planes / sparse_planes: bits,
    or ghf.RAW_AUTO / ghf.SPARSE_AUTO.  Waits for the device as often as ghf.Context.compress_planes_forms does for the same
    masks.  -> (d_container uint8, nbytes int64[1] device: the container's size, also when cap did not suffice)"""
    L = lib()
    if n_elems is None:
        n_elems = d_in.numel() * d_in.element_size() // elem_bytes
    d_container, cap, nbytes = _container(ctx, n_elems, elem_bytes, d_container, cap, nbytes)
    ctx._chk(L.ghf_compress_tensor(ctx.h, d_in.data_ptr(), _addr(d_base), n_elems, elem_bytes, raw_planes, sparse_planes,
                                   d_container.data_ptr(), cap, nbytes.data_ptr()), "ghf_compress_tensor")
    return d_container, nbytes


def release_workspace(ctx):
    """give back the device memory compress_tensor grew on ctx (about 2.25 times the largest tensor); waits for the stream"""
    ctx._chk(lib().ghf_tensor_workspace_release(ctx.h), "ghf_tensor_workspace_release")


def pack(ctx, streams, d_stream_bytes, indexes, ranks, raw_planes, sparse_planes, n_vals, n_elems, elem_bytes, flags=0, d_container=None,
         cap=None, nbytes=None):
    """what ghf.Context.compress_planes_forms left -> one container, without a wait.  streams: 2 * elem_bytes CUDA uint8
    tensors or addresses (None for an empty slot); d_stream_bytes: its out_bytes (device); indexes: its live side-cars (an
    Index array); ranks: per plane the rank table as a CUDA tensor or address, or None (the whole argument may be None without
    sparse planes).  -> (d_container, nbytes)"""
    L = lib()
    d_container, cap, nbytes = _container(ctx, n_elems, elem_bytes, d_container, cap, nbytes)
    e = elem_bytes
    h_streams = (C.c_void_p * (2 * e))(*[_addr(x) for x in list(streams)[: 2 * e]])
    h_ranks = None if ranks is None else (C.c_void_p * e)(*[_addr(x) for x in list(ranks)[:e]])
    h_n_vals = (C.c_size_t * e)(*[int(v) for v in list(n_vals)[:e]])
    ctx._chk(L.ghf_tensor_pack(ctx.h, h_streams, _addr(d_stream_bytes), indexes, h_ranks, raw_planes, sparse_planes, h_n_vals, n_elems, e,
                               flags, d_container.data_ptr(), cap, nbytes.data_ptr()), "ghf_tensor_pack")
    return d_container, nbytes


def open(ctx, d_container, container_bytes, head=None):  # noqa: A001 -- the module's verb, as the C call's
    """ghf_tensor_open: head = the container's first HEAD_BYTES as host bytes (None: the call fetches them and waits).
    Waits for the device only when a plane is sparse.  -> Tensor; raises GhfError (status 6, nothing queued) for a head
    that is not one of a container of container_bytes bytes"""
    L = lib()
    h = C.c_void_p()
    if head is None:
        rc = L.ghf_tensor_open(ctx.h, None, 0, _addr(d_container), container_bytes, C.byref(h))
    else:
        buf, n = _host(head)
        rc = L.ghf_tensor_open(ctx.h, buf, n, _addr(d_container), container_bytes, C.byref(h))
    if rc:
        assert not h.value
        ctx._chk(rc, "ghf_tensor_open")
    return Tensor(ctx, h, d_container)


class Tensor:
    """an opened container (ghf_tensor): decode, decode_range, gather, close.  Keeps the container's tensor referenced."""

    def __init__(self, ctx, handle, d_container):
        self.ctx, self.h, self.d_container = ctx, handle, d_container
        self.info = TensorInfo()
        ctx._chk(lib().ghf_tensor_describe(self.h, C.byref(self.info)), "ghf_tensor_describe")
        self.n_elems, self.elem_bytes = int(self.info.n_elems), int(self.info.elem_bytes)

    def close(self):
        if getattr(self, "h", None):
            lib().ghf_tensor_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def decode(self, d_base=None, d_out=None, cap=None, nbytes=None):
        """the whole tensor (XOR d_base for a DELTA container; d_out may be d_base).  Never waits.
        -> (d_out uint8, nbytes int64[1] device)"""
        ctx, t = self.ctx, self.ctx.torch
        if d_out is None:
            d_out = ctx.empty_u8(self.n_elems * self.elem_bytes)
        if nbytes is None:
            nbytes = t.zeros(1, dtype=t.int64, device=ctx.device)
        ctx._chk(lib().ghf_tensor_decode(ctx.h, self.h, _addr(d_base), d_out.data_ptr(), d_out.numel() if cap is None else cap,
                                         nbytes.data_ptr()), "ghf_tensor_decode")
        return d_out, nbytes

    def decode_range(self, first, count, d_base=None, d_out=None, cap=None):
        """elements [first, first + count); d_base: the base elements of the range itself, indexed like d_out.  -> d_out"""
        ctx = self.ctx
        if d_out is None:
            d_out = ctx.empty_u8(count * self.elem_bytes)
        ctx._chk(lib().ghf_tensor_decode_range(ctx.h, self.h, _addr(d_base), first, count, d_out.data_ptr(),
                                               d_out.numel() if cap is None else cap), "ghf_tensor_decode_range")
        return d_out

    def gather(self, d_index, row_elems, index_stride=None, d_base=None, n_rows=None, d_out=None, out_stride=None, d_row_status=None):
        """rows [d_index[r] * index_stride, + row_elems) in ONE launch; d_base: the WHOLE base tensor of a DELTA container.
        -> (d_out, d_row_status int32[n_rows])"""
        ctx, t = self.ctx, self.ctx.torch
        n_rows = d_index.numel() if n_rows is None else n_rows
        index_stride = row_elems if index_stride is None else index_stride
        out_stride = row_elems * self.elem_bytes if out_stride is None else out_stride
        if d_out is None:
            d_out = ctx.empty_u8(max(n_rows, 1) * out_stride)
        if d_row_status is None:
            d_row_status = t.zeros(max(n_rows, 1), dtype=t.int32, device=ctx.device)
        ctx._chk(lib().ghf_tensor_gather(ctx.h, self.h, _addr(d_base), d_index.data_ptr(), index_stride, row_elems, n_rows, d_out.data_ptr(),
                                         out_stride, d_row_status.data_ptr()), "ghf_tensor_gather")
        return d_out, d_row_status
