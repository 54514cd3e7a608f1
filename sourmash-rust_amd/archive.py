"""Zip collections of signatures -- the container sourmash writes its databases in -- loaded on the device (additive ABI
smh_archive_*): the compressed file is uploaded once and the chosen members are inflated in HBM, each into
its own slice of one text that signature.SignatureScan.parse takes.

    zc = archive.ZipCollection("gtdb-k31.zip")
    text, doc_offsets = zc.text(zc.select(ksize=31))
    index = ResidentIndex.from_zip("gtdb-k31.zip", ksize=31)

Members are `signatures/<md5>.sig.gz`, stored in the zip because they are gzip already, and a SOURMASH-MANIFEST.csv; plain
`.sig` members, deflated members and archives without a manifest are read as well.  The manifest is read on the host: it is
one member and can be tens of megabytes, the worst case for a decoder that gives a member one wave."""
import collections
import csv
import gzip
import io
import os
import zlib
import ctypes as C

import numpy as np

from ._lib import SmhArchiveEntry, lib, u32p, u64p
from .errors import SourmashError, call

KINDS = ("stored", "deflate", "gzip", "directory", "other")
MANIFEST = "SOURMASH-MANIFEST.csv"
# The text size above which a member is inflated on the host instead.  A lone member takes its one wave 14 MB/s, some 50 times
# what one host thread needs for zlib and the upload at every size measured, so no size passes a lone-member comparison; what
# counts is whether the member hides under the rest of the call.  256 KiB take a wave 19 ms, half of what the text of a
# collection of 8 000 sketches takes; 2 MB take 150 ms and were measured to hold such a call up (DESIGN.md 3.29 has the sweep).
DEFAULT_DEVICE_MEMBER_LIMIT = 1 << 18
# statuses with which a gzip member that is really several members comes back (ISIZE is the last member's): the host finishes it
_OUTPUT_OVER, _OUTPUT_UNDER, _LEFTOVER = 11, 12, 13

ArchiveEntry = collections.namedtuple("ArchiveEntry", "name method flags crc32 comp_size size header_off data_off kind device_ok reason "
                                                      "payload_off payload_len text_size text_crc")


class ZipCollection:
    """The entries of a zip archive, scanned on the host (smh_archive_scan; no device is touched), and its manifest.

    `entries` has one ArchiveEntry per central-directory entry, in directory order; `kind` is decided from content (stored,
    deflate, gzip, directory, other) and `device_ok` says whether the device can inflate it (`reason` says why not).
    `manifest` holds the rows of SOURMASH-MANIFEST.csv as dicts, or None."""

    def __init__(self, source):
        self._L = lib()
        if isinstance(source, (bytes, bytearray, memoryview)):
            self.data = bytes(source)
        else:
            with open(source, "rb") as fh:
                self.data = fh.read()
        self._p = call(self._L.smh_archive_scan, self.data, len(self.data))
        out, e = [], SmhArchiveEntry()
        for i in range(self._L.smh_archive_entries(self._p)):
            call(self._L.smh_archive_entry, self._p, i, C.byref(e))
            out.append(ArchiveEntry(e.name.decode("utf-8", "replace"), e.method, e.flags, e.crc32, e.comp_size, e.size, e.header_off, e.data_off,
                                    KINDS[e.kind], bool(e.device_ok), e.reason.decode(), e.payload_off, e.payload_len, e.text_size, e.text_crc))
        self.entries = out
        self._by_name = {}
        for i, en in enumerate(out):
            self._by_name.setdefault(en.name, i)
        self.manifest = self._read_manifest()

    def __del__(self):
        try:
            self._L.smh_archive_free(self._p)
        except Exception:
            pass

    def __len__(self): return len(self.entries)

    def read(self, i):
        """entry i's content, decompressed on the host (the zip layer only: a stored .sig.gz comes back as gzip)"""
        e = self.entries[i]
        if e.flags & 1:
            raise ValueError("entry %d %r is encrypted" % (i, e.name))
        raw = self.data[e.data_off:e.data_off + e.comp_size]
        if e.method == 0:
            return raw
        if e.method == 8:
            return zlib.decompress(raw, -15)
        raise ValueError("entry %d %r: compression method %d" % (i, e.name, e.method))

    def _read_manifest(self):
        i = self._by_name.get(MANIFEST)
        if i is None:
            return None
        raw = self.read(i)
        if raw[:2] == b"\x1f\x8b":
            raw = gzip.decompress(raw)
        lines = raw.decode("utf-8")
        if lines.startswith("# SOURMASH-MANIFEST-VERSION"):
            lines = lines[lines.index("\n") + 1:] if "\n" in lines else ""
        return list(csv.DictReader(io.StringIO(lines, newline="")))

    def select(self, ksize=0, moltype=None, md5=None, names=None):
        """Entry ids, each once.  With a manifest: the `internal_location` of every row that passes ksize (0: any), moltype
        (None: any; compared without case), md5 (a string or a collection of them) and names (a collection of member names),
        in manifest order.  Without one: every non-directory entry whose name ends .sig or .sig.gz, in directory order, that
        passes `names` -- what is inside is only known once it is read (ResidentIndex.from_zip filters the sketches)."""
        md5s = None if md5 is None else ({md5} if isinstance(md5, str) else set(md5))
        names = None if names is None else set(names)
        out, seen = [], set()
        if self.manifest is not None:
            for row in self.manifest:
                if ksize and int(row.get("ksize") or 0) != int(ksize):
                    continue
                if moltype is not None and (row.get("moltype") or "").lower() != moltype.lower():
                    continue
                if md5s is not None and row.get("md5") not in md5s:
                    continue
                loc = row.get("internal_location")
                if names is not None and loc not in names:
                    continue
                if loc not in self._by_name:
                    raise ValueError("the manifest names %r, which the archive does not hold" % (loc,))
                i = self._by_name[loc]
                if i not in seen:
                    seen.add(i)
                    out.append(i)
            return out
        for i, e in enumerate(self.entries):
            if e.kind != "directory" and (e.name.endswith(".sig") or e.name.endswith(".sig.gz")) and (names is None or e.name in names):
                out.append(i)
        return out

    def _host_text(self, i):
        content = self.read(i)
        return gzip.decompress(content) if content[:2] == b"\x1f\x8b" else content

    def _doubly_compressed(self, e):
        """a deflate entry whose text itself begins 1f 8b: the first two bytes, by the host.  A stream zlib cannot start is not
        doubly compressed: the device takes it and reports what is wrong with it"""
        try:
            head = zlib.decompressobj(-15).decompress(self.data[e.data_off:e.data_off + e.comp_size], 2)
        except zlib.error:
            return False
        return head == b"\x1f\x8b"

    def text(self, ids=None, device_member_limit=None, verify=True, stream=None, status=None):
        """(text, doc_offsets): the chosen entries' signature JSON one after another as a CUDA uint8 tensor, and len(ids) + 1
        offsets, as SignatureScan.parse takes them.  ids None: select().  Everything goes through ONE device call
        (smh_archive_inflate: one upload of the compressed file) except the entries the host finishes, copied into their
        slices: entries with device_ok false, entries whose text is larger than device_member_limit (None: the default),
        deflate entries whose content is itself gzip, and gzip entries that are really several members (the device reports
        them; the call is then made again without them).  verify: check every text's CRC-32.  status: a numpy uint8 array of
        one entry per id that receives the device's status per id (0 for the ones the host took)."""
        import torch
        L = self._L
        ids = self.select() if ids is None else [int(i) for i in ids]
        limit = DEFAULT_DEVICE_MEMBER_LIMIT if device_member_limit is None else int(device_member_limit)
        n = len(ids)
        for i in ids:
            if not 0 <= i < len(self.entries):
                raise ValueError("entry %d of %d" % (i, len(self.entries)))
        if not L.smh_device_available():
            call(L.smh_archive_inflate, self._p, self.data, len(self.data), None, None, 0, None, 0, 1, None)   # raises: no device
        host = {}                                           # position -> bytes
        for k, i in enumerate(ids):
            e = self.entries[i]
            if not e.device_ok or e.text_size > limit or (e.kind == "deflate" and self._doubly_compressed(e)):
                host[k] = self._host_text(i)
        while True:
            sizes = np.array([len(host[k]) if k in host else self.entries[i].text_size for k, i in enumerate(ids)], dtype=np.uint64)
            offs = np.zeros(n + 1, dtype=np.uint64)
            np.cumsum(sizes, out=offs[1:])
            total = int(offs[-1])
            out = torch.empty(total, dtype=torch.uint8, device="cuda")
            pos = [k for k in range(n) if k not in host]
            st = np.zeros(max(len(pos), 1), dtype=np.uint8)
            if pos:
                dev_ids = np.array([ids[k] for k in pos], dtype=np.uint32)
                dev_offs = np.ascontiguousarray(offs[pos], dtype=np.uint64)
                args = (dev_ids.ctypes.data_as(u32p), dev_offs.ctypes.data_as(u64p), len(pos), C.c_void_p(out.data_ptr() if total else 0),
                        total, int(bool(verify)), st.ctypes.data_as(C.POINTER(C.c_uint8)))
                try:
                    if stream is None:
                        call(L.smh_archive_inflate, self._p, self.data, len(self.data), *args)
                    else:
                        comp = torch.frombuffer(bytearray(self.data), dtype=torch.uint8).cuda()
                        torch.cuda.current_stream().synchronize()
                        call(L.smh_archive_inflate_dev, self._p, C.c_void_p(comp.data_ptr()), comp.numel(), *args, C.c_void_p(stream))
                except SourmashError as err:
                    bad = [k for k, s in zip(pos, st) if s]
                    again = [k for k in bad if self.entries[ids[k]].kind == "gzip" and st[pos.index(k)] in (_OUTPUT_OVER, _OUTPUT_UNDER, _LEFTOVER)]
                    if err.code != 3 or not bad or len(again) != len(bad):
                        if status is not None:
                            status[:] = 0
                            status[pos] = st[:len(pos)]
                        raise
                    for k in again:                         # several gzip members in one entry: the host's gzip reads them all
                        host[k] = self._host_text(ids[k])
                    continue
            break
        if status is not None:
            status[:] = 0
            status[pos] = st[:len(pos)]
        for k, content in host.items():
            if content:
                out[int(offs[k]):int(offs[k + 1])].copy_(torch.frombuffer(bytearray(content), dtype=torch.uint8))
        if host:
            torch.cuda.current_stream().synchronize()
        return out, offs


def is_zip(source):
    """True when the bytes, or the file at the path, begin with a local file header (PK\\3\\4)"""
    if isinstance(source, (bytes, bytearray, memoryview)):
        return bytes(source[:4]) == b"PK\x03\x04"
    if isinstance(source, (str, os.PathLike)):
        try:
            with open(source, "rb") as fh:
                return fh.read(4) == b"PK\x03\x04"
        except OSError:
            return False
    return False
