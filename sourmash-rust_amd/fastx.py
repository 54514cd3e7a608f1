"""FASTA / FASTQ text -> records, parsed on the device (additive ABI smh_records_*).

    recs = fastx.Records.parse(fastx.read_text("reads.fastq.gz"))
    mh.add_records(recs)
    prot.add_records_protein(fastx.Records.parse(fastx.read_text("proteome.faa")))     # amino acids: a protein / dayhoff / hp sketch

The text may be host bytes (uploaded, then parsed) or a CUDA uint8 tensor already in HBM.  The handle owns the
compacted sequence bytes and the offsets; it keeps no reference to the text.  Names are spans into the text: the
library copies none, `names(text)` slices them out of the caller's own copy."""
import ctypes as C
import gzip

import numpy as np

from ._lib import lib, u64p
from .errors import call

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


class _DeviceSpan:
    """`nbytes` of device memory at `ptr` as something torch.as_tensor can view."""
    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2,
                                         "strides": None}


class Records:
    def __init__(self, ptr):
        self._L = lib()
        self._p = ptr

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

    def names(self, text):
        """The names, cut out of the caller's host copy of the text."""
        text = bytes(text)
        start, length = self.name_spans()
        return [text[int(s):int(s) + int(l)] for s, l in zip(start, length)]

    def seq_tensor(self):
        """The compacted sequence bytes as a CUDA uint8 tensor of its own (a device-to-device copy)."""
        import torch
        n = self.total
        if n == 0:
            return torch.empty(0, dtype=torch.uint8, device="cuda")
        view = torch.as_tensor(_DeviceSpan(self._L.smh_records_seq_dev(self._p), n), device="cuda")
        return view.clone()
