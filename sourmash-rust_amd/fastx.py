"""FASTA / FASTQ text -> records, parsed on the device (additive ABI smh_records_*), and blocked gzip
(BGZF) inflated on the device in front of it (smh_gzip_*).

    recs = fastx.Records.parse(fastx.read_text("reads.fastq.gz"))
    recs = fastx.Records.parse(fastx.read_device_text("reads.fastq.gz"))               # bgzip output: inflated in HBM
    mh.add_records(recs)
    prot.add_records_protein(fastx.Records.parse(fastx.read_text("proteome.faa")))     # amino acids: a protein / dayhoff / hp sketch

The text may be host bytes (uploaded, then parsed) or a CUDA uint8 tensor already in HBM.  The handle owns the
compacted sequence bytes and the offsets; it keeps no reference to the text.  Names are spans into the text: the
library copies none, `names(text)` slices them out of the caller's own copy."""
import ctypes as C
import gzip

import numpy as np

from ._lib import lib, u64p
from .errors import SourmashError, call

FORMATS = {"auto": 0, "fasta": 1, "fastq": 2}
_NAMES = {v: k for k, v in FORMATS.items()}


def read_text(path):
    """The file's bytes; through Python's gzip when it begins with 1f 8b.  Decompression stays on the host."""
    with open(path, "rb") as fh:
        magic = fh.read(2)
    if magic == b"\x1f\x8b":
        with gzip.open(path, "rb") as fh:
            return fh.read()
    with open(path, "rb") as fh:
        return fh.read()


class GzipMembers:
    """The member table of a blocked-gzip (BGZF) chain, found on the host by hopping headers (smh_gzip_scan)."""
    def __init__(self, data):
        self._L = lib()
        data = bytes(data)
        self.nbytes = len(data)
        self._p = call(self._L.smh_gzip_scan, data, len(data))

    def __del__(self):
        try:
            self._L.smh_gzip_free(self._p)
        except Exception:
            pass

    def __len__(self): return self._L.smh_gzip_members(self._p)

    @property
    def inflated_len(self): return self._L.smh_gzip_inflated_len(self._p)

    def member(self, i):
        """(payload offset, payload length, ISIZE, CRC-32) of member i"""
        off, plen, isize, crc = C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        call(self._L.smh_gzip_member, self._p, i, C.byref(off), C.byref(plen), C.byref(isize), C.byref(crc))
        return off.value, plen.value, isize.value, crc.value


def gzip_scan(data):
    """The members of blocked gzip; SourmashError (code 3) names the member and its byte offset when the bytes are not
    gzip, not blocked gzip ("not blocked gzip": fall back to the host), cut short or followed by other bytes."""
    return GzipMembers(data)


def is_bgzf(data):
    """True when the bytes begin with a gzip member that carries the BC subfield (the whole chain is not walked)."""
    data = bytes(data[:65536])
    if len(data) < 18 or data[:3] != b"\x1f\x8b\x08" or not data[3] & 4:
        return False
    xlen = data[10] | data[11] << 8
    at, end = 12, min(12 + xlen, len(data))
    while at + 4 <= end:
        slen = data[at + 2] | data[at + 3] << 8
        if data[at:at + 2] == b"BC" and slen == 2:
            return True
        at += 4 + slen
    return False


def inflate(data, verify=True, stream=None, members=None, status=None):
    """Blocked gzip -> its text as a CUDA uint8 tensor, inflated on the device.  data: host bytes, or a
    contiguous one-dimensional CUDA uint8 tensor of the compressed bytes together with members=gzip_scan(the same bytes).
    verify: check every member's CRC-32 (its size is always checked).  status: a numpy uint8 array of one entry per member
    that receives each member's reason (0: ok), also when the call raises for the lowest bad member."""
    import torch
    L = lib()
    on_device = hasattr(data, "data_ptr")
    if on_device:
        if members is None:
            raise ValueError("compressed bytes in device memory need members=gzip_scan(...) of the same bytes")
        if not data.is_cuda or data.dim() != 1 or not data.is_contiguous() or data.element_size() != 1:
            raise ValueError("device data must be a contiguous one-dimensional CUDA uint8 tensor")
    else:
        data = bytes(data)
        if members is None:
            members = gzip_scan(data)
    n = len(members)
    if status is not None and (status.dtype != np.uint8 or status.size != n or not status.flags.c_contiguous):
        raise ValueError("status must be a contiguous numpy uint8 array of one entry per member")
    sp = status.ctypes.data_as(C.POINTER(C.c_uint8)) if status is not None and n else None
    if not L.smh_device_available():
        call(L.smh_gzip_inflate, b"", 0, None, 0, 1, None)     # raises: no device
    out = torch.empty(members.inflated_len, dtype=torch.uint8, device="cuda")
    op = C.c_void_p(out.data_ptr() if out.numel() else 0)
    if on_device:
        call(L.smh_gzip_inflate_dev, members._p, C.c_void_p(data.data_ptr() if data.numel() else 0), data.numel(), op, out.numel(),
             int(bool(verify)), sp, C.c_void_p(stream or 0))
    elif stream is None:
        call(L.smh_gzip_inflate, data, len(data), op, out.numel(), int(bool(verify)), sp)
    else:
        comp = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda() if data else torch.empty(0, dtype=torch.uint8, device="cuda")
        torch.cuda.current_stream().synchronize()
        call(L.smh_gzip_inflate_dev, members._p, C.c_void_p(comp.data_ptr() if comp.numel() else 0), comp.numel(), op, out.numel(),
             int(bool(verify)), sp, C.c_void_p(stream))
    return out


def read_device_text(path):
    """The file's text as a CUDA uint8 tensor.  Blocked gzip is uploaded compressed and inflated on the device; other gzip
    goes through Python's gzip on the host and is uploaded as text; anything else is uploaded as it is."""
    import torch
    with open(path, "rb") as fh:
        data = fh.read()
    if is_bgzf(data):
        try:
            return inflate(data)
        except SourmashError as e:                       # a chain that goes on as plain gzip: the scan says so, the host takes it
            if e.code != 3 or "not blocked gzip" not in e.message:
                raise
    if data[:2] == b"\x1f\x8b":
        data = gzip.decompress(data)
    if not data:
        return torch.empty(0, dtype=torch.uint8, device="cuda")
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


class _DeviceSpan:
    """`nbytes` of device memory at `ptr` as something torch.as_tensor can view."""
    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2,
                                         "strides": None}


class Records:
    def __init__(self, ptr):
        self._L = lib()
        self._p = ptr
        self.text = None            # the device text, when parse_bgzf was asked to keep it

    def __del__(self):
        try:
            self._L.smh_records_free(self._p)
        except Exception:
            pass

    @classmethod
    def parse(cls, text, format="auto", stream=None):
        """text: bytes-like (host) or a contiguous one-dimensional CUDA uint8 tensor.  format: auto, fasta or fastq."""
        fmt = FORMATS[format] if isinstance(format, str) else int(format)
        L = lib()
        if hasattr(text, "data_ptr"):
            if not text.is_cuda or text.dim() != 1 or not text.is_contiguous() or text.element_size() != 1:
                raise ValueError("a device text must be a contiguous one-dimensional CUDA uint8 tensor")
            n = text.numel()
            p = call(L.smh_records_parse_dev, C.c_void_p(text.data_ptr() if n else 0), n, fmt, C.c_void_p(stream or 0))
        else:
            text = bytes(text)
            p = call(L.smh_records_parse, text, len(text), fmt)
        return cls(p)

    @classmethod
    def parse_bgzf(cls, data, format="auto", keep_text=False, stream=None):
        """Blocked gzip (host bytes) inflated on the device and parsed there: the text never exists on the host."""
        text = inflate(data, stream=stream)
        recs = cls.parse(text, format, stream)
        if keep_text:
            recs.text = text
        return recs

    def __len__(self): return self._L.smh_records_len(self._p)

    @property
    def total(self): return self._L.smh_records_total(self._p)

    @property
    def format(self): return _NAMES[self._L.smh_records_format(self._p)]

    @property
    def offsets(self):
        """n + 1 offsets into the compacted bytes (a copy)."""
        p = self._L.smh_records_offsets(self._p)
        return np.ctypeslib.as_array(p, shape=(len(self) + 1,)).copy()

    def name_spans(self):
        """(start, length) of every record's name in the text that was parsed."""
        n = len(self)
        start, length = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint32)
        call(self._L.smh_records_names, self._p, start.ctypes.data_as(u64p), length.ctypes.data_as(C.POINTER(C.c_uint32)))
        return start, length

    def names(self, text=None):
        """The names, cut out of the caller's host copy of the text.  Without an argument: out of the device text that
        parse_bgzf(keep_text=True) kept -- the name bytes are gathered on the device and only they are read back."""
        start, length = self.name_spans()
        if text is None:
            if self.text is None:
                raise ValueError("names() needs the text: pass it, or parse with parse_bgzf(keep_text=True)")
            import torch
            n = np.cumsum(length, dtype=np.int64)
            total = int(n[-1]) if len(n) else 0
            if total == 0:
                return [b""] * len(length)
            lens = torch.from_numpy(length.astype(np.int64)).cuda()
            first = torch.from_numpy(start.astype(np.int64) - (n - length)).cuda()      # start of the span - its place in the gather
            idx = torch.repeat_interleave(first, lens) + torch.arange(total, device="cuda")
            flat = self.text[idx].cpu().numpy().tobytes()
            return [flat[int(e) - int(l):int(e)] for e, l in zip(n, length)]
        text = bytes(text)
        return [text[int(s):int(s) + int(l)] for s, l in zip(start, length)]

    def seq_tensor(self):
        """The compacted sequence bytes as a CUDA uint8 tensor of its own (a device-to-device copy)."""
        import torch
        n = self.total
        if n == 0:
            return torch.empty(0, dtype=torch.uint8, device="cuda")
        view = torch.as_tensor(_DeviceSpan(self._L.smh_records_seq_dev(self._p), n), device="cuda")
        return view.clone()
