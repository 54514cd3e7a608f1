"""Host-side mirror of the reference's Signature (src/lib.rs:546-675) over the C ABI
(src/ffi.rs:327-604)."""
import collections
import ctypes as C
import gzip
import os

import numpy as np

from ._lib import SmhSigEntry, lib, u64p
from .errors import SourmashError, call, take_str
from .minhash import MOLECULES, KmerMinHash


class Signature:
    def __init__(self, _ptr=None):
        self._L = lib()
        self._p = _ptr if _ptr is not None else self._L.signature_new()

    def __del__(self):
        try:
            self._L.signature_free(self._p)
        except Exception:
            pass

    @property
    def name(self): return take_str(call(self._L.signature_get_name, self._p)).decode()
    @name.setter
    def name(self, v): call(self._L.signature_set_name, self._p, v.encode())
    @property
    def filename(self): return take_str(call(self._L.signature_get_filename, self._p)).decode()
    @filename.setter
    def filename(self, v): call(self._L.signature_set_filename, self._p, v.encode())
    @property
    def license(self): return take_str(call(self._L.signature_get_license, self._p)).decode()

    def push_mh(self, mh): call(self._L.signature_push_mh, self._p, mh._p)
    def set_mh(self, mh): call(self._L.signature_set_mh, self._p, mh._p)
    def first_mh(self): return KmerMinHash(0, 0, _ptr=call(self._L.signature_first_mh, self._p))

    def sketches(self):
        n = C.c_size_t()
        arr = call(self._L.signature_get_mhs, self._p, C.byref(n))
        return [KmerMinHash(0, 0, _ptr=arr[i]) for i in range(n.value)]

    def save_json(self): return take_str(call(self._L.signature_save_json, self._p)).decode()
    def __eq__(self, other): return bool(call(self._L.signature_eq, self._p, other._p))


def _wrap(arr, n):
    return [Signature(_ptr=arr[i]) for i in range(n)]


def load_signatures_buffer(data, ksize=0, moltype=None):
    """reference Signature::load_signatures via signatures_load_buffer (one Signature per sketch)."""
    n = C.c_size_t()
    arr = call(lib().signatures_load_buffer, data, len(data), False, ksize,
               moltype.encode() if moltype else None, C.byref(n))
    return _wrap(arr, n.value)


def load_signatures_path(path, ksize=0, moltype=None):
    n = C.c_size_t()
    arr = call(lib().signatures_load_path, path.encode(), False, ksize,
               moltype.encode() if moltype else None, C.byref(n))
    return _wrap(arr, n.value)


def from_json(data):
    """Signature::from_reader view (no flattening).  The reference ABI only exposes the flattened
    load, so each top-level element is loaded on its own and its sketches pushed back together."""
    import json
    docs = json.loads(data)
    if not isinstance(docs, list):
        load_signatures_buffer(data)  # let the library raise its serde error
    out = []
    for d in docs:
        flat = load_signatures_buffer(json.dumps([d]).encode())
        if not flat:
            out.append(Signature())
            continue
        s = flat[0]
        for extra in flat[1:]:
            s.push_mh(extra.first_mh())
        out.append(s)
    return out


SPAN_STATUS = ("closed", "open", "overflow", "bad_syntax")
SigEntry = collections.namedtuple("SigEntry", "document signature sketch name filename license sig_class md5sum num ksize seed max_hash "
                                              "molecule n_mins has_abundances n_abundances mins_span abundances_span")


class SignatureScan:
    """Signature JSON read on the device (additive ABI smh_signatures_*): every number of every numeric array
    of the text as u64 in HBM, the span table and every sketch's metadata on the host.

        scan = SignatureScan.parse(open("db.sig", "rb").read())
        index = ResidentIndex.from_signatures(scan, ksize=31)

    `entries` has one SigEntry per sketch, in the order load_signatures_buffer flattens them; name / filename are None for a
    JSON null.  The handle keeps no reference to the text."""

    def __init__(self, ptr):
        self._L = lib()
        self._p = ptr
        self._entries = None

    def __del__(self):
        try:
            self._L.smh_signatures_free(self._p)
        except Exception:
            pass

    @classmethod
    def parse(cls, data, doc_offsets=None, stream=None):
        """data: bytes-like (host; uploaded once) or a contiguous one-dimensional CUDA uint8 tensor.  doc_offsets: len + 1
        ascending offsets, document d = data[doc_offsets[d]:doc_offsets[d + 1]], each a JSON array of signatures; None: the
        whole text is one document.  A document the host loader refuses raises SourmashError (code 100004) naming the
        document and the byte; a number with a fraction or an exponent inside an array raises code 3."""
        L = lib()
        offs, n_docs, op = None, 0, None
        if doc_offsets is not None:
            offs = np.ascontiguousarray(doc_offsets, dtype=np.uint64)
            if offs.ndim != 1 or offs.size < 1:
                raise ValueError("doc_offsets: one more entry than documents")
            n_docs, op = offs.size - 1, offs.ctypes.data_as(u64p)
        if hasattr(data, "data_ptr"):
            if not data.is_cuda or data.dim() != 1 or not data.is_contiguous() or data.element_size() != 1:
                raise ValueError("a device text must be a contiguous one-dimensional CUDA uint8 tensor")
            n = data.numel()
            p = call(L.smh_signatures_parse_dev, C.c_void_p(data.data_ptr() if n else 0), n, op, n_docs, C.c_void_p(stream or 0))
        else:
            data = bytes(data)
            p = call(L.smh_signatures_parse, data, len(data), op, n_docs)
        return cls(p)

    def __len__(self): return self._L.smh_signatures_len(self._p)

    @property
    def n_spans(self): return self._L.smh_signatures_spans(self._p)

    @property
    def n_tokens(self): return self._L.smh_signatures_tokens(self._p)

    @property
    def entries(self):
        if self._entries is None:
            out, e = [], SmhSigEntry()
            for i in range(len(self)):
                call(self._L.smh_signatures_entry, self._p, i, C.byref(e))
                out.append(SigEntry(e.document, e.signature, e.sketch, None if e.name_is_null else e.name.decode(),
                                    None if e.filename_is_null else e.filename.decode(), e.license.decode(), e.sig_class.decode(),
                                    e.md5sum.decode(), e.num, e.ksize, e.seed, e.max_hash, MOLECULES[e.molecule], e.n_mins,
                                    bool(e.has_abundances), e.n_abundances, e.mins_span, e.abundances_span if e.has_abundances else None))
            self._entries = out
        return self._entries

    def spans(self):
        """the span table: a list of dicts with start, end, first_token, n_tokens, status (0 closed, 1 open, 2 overflow,
        3 bad syntax) and bad_off (2^64 - 1: none)"""
        out = []
        v = [C.c_uint64() for _ in range(5)]
        st = C.c_uint32()
        for k in range(self.n_spans):
            call(self._L.smh_signatures_span, self._p, k, C.byref(v[0]), C.byref(v[1]), C.byref(v[2]), C.byref(v[3]), C.byref(st), C.byref(v[4]))
            out.append({"start": v[0].value, "end": v[1].value, "first_token": v[2].value, "n_tokens": v[3].value, "status": st.value,
                        "bad_off": v[4].value})
        return out

    def values(self):
        """every token's value as a CUDA int64 tensor of its own (the u64 bit patterns; a device-to-device copy)"""
        import torch
        from .fastx import _DeviceSpan
        n = self.n_tokens
        if n == 0:
            return torch.empty(0, dtype=torch.int64, device="cuda")
        view = torch.as_tensor(_DeviceSpan(self._L.smh_signatures_values_dev(self._p), n * 8), device="cuda")
        return view.clone().view(torch.int64)


class SigText:
    """Signature JSON written on the device (additive ABI smh_index_sigtext, smh_sigtext_*): the text of a
    resident index in HBM, owned by this handle.  ResidentIndex.save_signatures makes one."""

    def __init__(self, ptr):
        self._L = lib()
        self._p = ptr

    def __del__(self):
        try:
            self._L.smh_sigtext_free(self._p)
        except Exception:
            pass

    def __len__(self): return self._L.smh_sigtext_len(self._p)

    @property
    def doc_offsets(self):
        """documents + 1 byte offsets from 0, as SignatureScan.parse takes them"""
        out = np.zeros(self._L.smh_sigtext_documents(self._p) + 1, dtype=np.uint64)
        call(self._L.smh_sigtext_doc_offsets, self._p, out.ctypes.data_as(u64p))
        return out

    def read(self, offset=0, length=None):
        """text[offset:offset + length] as bytes (smh_sigtext_read)"""
        length = len(self) - offset if length is None else length
        buf = C.create_string_buffer(max(length, 1))
        call(self._L.smh_sigtext_read, self._p, offset, length, buf)
        return buf.raw[:length]

    def tensor(self):
        """the text as a CUDA uint8 tensor of its own (a device-to-device copy)"""
        import torch
        from .fastx import _DeviceSpan
        n = len(self)
        if n == 0:
            return torch.empty(0, dtype=torch.uint8, device="cuda")
        return torch.as_tensor(_DeviceSpan(self._L.smh_sigtext_dev(self._p), n), device="cuda").clone()

    def view(self):
        """the text in place as a CUDA uint8 tensor; valid only while this handle lives"""
        import torch
        from .fastx import _DeviceSpan
        return torch.as_tensor(_DeviceSpan(self._L.smh_sigtext_dev(self._p), max(len(self), 1)), device="cuda")[:len(self)]


def read_signature_text(paths):
    """The text of one .sig file or of several, one after another, as (data, doc_offsets): a CUDA uint8 tensor when a file is
    blocked gzip (it is inflated on the device, fastx.inflate), else host bytes.  Plain files and single-stream gzip are read
    on the host."""
    from . import fastx
    if isinstance(paths, (str, bytes, os.PathLike)):
        paths = [paths]
    parts, on_device = [], False
    for path in paths:
        with open(path, "rb") as fh:
            raw = fh.read()
        if fastx.is_bgzf(raw):
            try:
                parts.append(fastx.inflate(raw))
                on_device = True
                continue
            except SourmashError as e:
                if e.code != 3 or "not blocked gzip" not in e.message:
                    raise
        parts.append(gzip.decompress(raw) if raw[:2] == b"\x1f\x8b" else raw)
    sizes = [p.numel() if hasattr(p, "data_ptr") else len(p) for p in parts]
    offs = np.zeros(len(parts) + 1, dtype=np.uint64)
    np.cumsum(np.array(sizes, dtype=np.uint64), out=offs[1:])
    if not on_device:
        return b"".join(parts), offs
    import torch
    dev = [p if hasattr(p, "data_ptr") else (torch.frombuffer(bytearray(p), dtype=torch.uint8).cuda() if p else
                                             torch.empty(0, dtype=torch.uint8, device="cuda")) for p in parts]
    return torch.cat(dev) if dev else torch.empty(0, dtype=torch.uint8, device="cuda"), offs


def save_signatures(sigs):
    arr = (C.c_void_p * max(len(sigs), 1))(*[s._p for s in sigs])
    return take_str(call(lib().signatures_save_buffer, arr, len(sigs))).decode()
