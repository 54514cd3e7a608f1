"""The zip scan, the shared DEFLATE decoder and the chunked CRC fold built for the host under the address and
undefined-behaviour sanitizers and run as a child process (tests/c_archive_host.cpp) on every crafted archive, every
truncation of a small valid one and 2 000 byte-level mutants of it: it must give the restatement's entries, refusals,
statuses and bytes, find the folded CRC equal to the serial one on every case, and end clean.  Nothing is preloaded and no
library is loaded into Python.  This is the gate in front of the malformed cases of tests/test_gpu_archive.py: the library and
the kernels compile the same source."""
import os
import struct
import subprocess
import zlib

import pytest

import archive_restatement as R
from conftest import ROOT

CSRC = os.path.join(ROOT, "sourmash-rust_amd", "csrc")


def big_cases():
    """texts at the chunk sizes where the fold changes shape, as deflated, stored and gzip entries"""
    C = R.CHUNK
    out = []
    for size in (0, 1, C - 1, C, C + 1, 2 * C + 1, 65 * C + 1, 65536, 65537):
        text = bytes((i * 7 + (i >> 9)) & 0xFF for i in range(size))
        out.append(("sizes_%d" % size, R.build([R.member("d.sig", text, 8), R.member("s.sig", text), R.member("g.sig.gz", R.gz(text)),
                                                  R.member("bad.sig", text, crc=zlib.crc32(text) ^ 0x8000)])))
    return out


def all_cases():
    cases = R.crafted() + big_cases()
    three = R.three()
    cases += [("cut_%d" % k, three[:k]) for k in range(len(three))]
    cases += [("mutant_%d" % k, m) for k, m in enumerate(R.mutants())]
    return cases


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("archive_host") / "c_archive_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "c_archive_host.cpp"), "-o", exe])
    return exe


def run_host(exe, cases, tmp_path):
    """per case: a refusal message, or [(Entry, status verified, status unverified, text)]"""
    src, dst = str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")
    with open(src, "wb") as fh:
        fh.write(struct.pack("<I", len(cases)))
        for _, data in cases:
            fh.write(struct.pack("<I", len(data)) + data)
    done = subprocess.run([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0 and "c archive host ok: %d cases" % len(cases) in done.stdout, done.stdout[-4000:]
    raw, at, out = open(dst, "rb").read(), 0, []

    def blob():
        nonlocal at
        n, = struct.unpack_from("<I", raw, at)
        at += 4 + n
        return raw[at - n:at]
    for _ in cases:
        ok, = struct.unpack_from("<I", raw, at)
        at += 4
        if not ok:
            out.append(blob().decode())
            continue
        n, = struct.unpack_from("<I", raw, at)
        at += 4
        rows = []
        for _ in range(n):
            name, reason = blob(), blob().decode()
            method, flags, crc32, kind, device_ok, text_size, text_crc, comp_size, size, header_off, data_off, payload_off, payload_len, sv, su = \
                struct.unpack_from("<7I6Q2I", raw, at)
            at += 7 * 4 + 6 * 8 + 2 * 4
            text = blob()
            rows.append((R.Entry(name, method, flags, crc32, comp_size, size, header_off, data_off, kind, bool(device_ok), reason, payload_off,
                                 payload_len, text_size, text_crc), sv, su, text))
        out.append(rows)
    assert at == len(raw)
    return out


def test_host_build_agrees_with_the_restatement(host_program, tmp_path):
    cases = all_cases()
    results = run_host(host_program, cases, tmp_path)
    refused, statuses, kinds = 0, set(), set()
    for (name, data), got in zip(cases, results):
        try:
            want = R.scan(data)
        except R.Refused as e:
            assert got == str(e), (name, got, str(e))
            refused += 1
            continue
        assert not isinstance(got, str), (name, got)
        assert [g[0] for g in got] == want, name
        for e, (_, sv, su, text) in zip(want, got):
            big = name.startswith("sizes_") and e.text_size > 4 * R.CHUNK   # (long valid texts: zlib stands in for the Python decoder)
            if big and e.device_ok:
                raw = data[e.payload_off:e.payload_off + e.payload_len]
                t = raw if e.kind == R.STORED else zlib.decompress(raw, -15)
                want_v, want_u, want_text = (R.IR.OK if zlib.crc32(t) == e.text_crc else R.IR.CRC), R.IR.OK, t
            else:
                want_text, want_v = R.status(data, e, True)
                _, want_u = R.status(data, e, False)
            assert (sv, su) == (want_v, want_u), (name, e.name, sv, su, want_v, want_u)
            assert text == want_text, (name, e.name)             # on a failure too: both stop at the same byte
            statuses.add(sv)
            kinds.add(e.kind)
    assert refused > 200 and kinds == {R.STORED, R.DEFLATE, R.GZIP, R.DIRECTORY, R.OTHER}
    assert statuses >= {R.IR.OK, R.IR.CRC, R.IR.LEFTOVER, R.IR.OUT_OVER, R.IR.OUT_UNDER, R.NOT_RUN}, sorted(statuses)
    # the archives tests/test_gpu_archive.py sends damaged members from are all among the cases above
    assert {"bad_mix", "host_served", "trailer_and_good", "equal_halves", "flipped_payload", "wrong_crc", "wrong_trailer",
            "gzip_two_members"} <= {name for name, _ in cases}


def test_the_header_needs_no_hip(tmp_path):
    """plain g++ compiles the header alone, with every warning an error"""
    src = tmp_path / "only.cpp"
    src.write_text('#include "archive_core.hpp"\nint main() { return smh::archive::chunks_of(smh::archive::kChunk + 1) == 2 ? 0 : 1; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", CSRC, str(src)])
