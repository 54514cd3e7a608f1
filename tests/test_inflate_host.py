"""The shared DEFLATE decoder built for the host under the address and undefined-behaviour sanitizers and run as a child
process on every crafted case and every fuzz mutant (tests/c_inflate_host.cpp): it must give the restatement's status and
bytes and end clean.  Nothing is preloaded and no library is loaded into Python.  This is the gate in front of the malformed
cases of tests/test_gpu_inflate.py: the kernel runs the same source."""
import os
import struct
import subprocess
import zlib

import pytest

import inflate_restatement as R
from conftest import ROOT


def all_cases():
    """[(name, payload, isize, crc, verify)]"""
    cases = [(name, p, len(t), zlib.crc32(t), 1) for name, p, t in R.valid_cases()]
    cases += [(name, p, isize, 0, 0) for name, p, isize, _ in R.malformed_cases()]
    text = R.fastq_text(5)
    cases += [("crc_flipped", R.deflate(text), len(text), zlib.crc32(text) ^ 0x10000, 1),
              ("crc_not_asked", R.deflate(text), len(text), zlib.crc32(text) ^ 0x10000, 0),
              ("empty_payload", b"", 0, 0, 1), ("empty_payload_isize", b"", 5, 0, 1)]
    cases += [("fuzz_%d" % i, p, isize, crc, 1) for i, (p, isize, crc) in enumerate(R.fuzz_mutants())]
    return cases


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("inflate_host") / "c_inflate_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "sourmash-rust_amd", "csrc"), os.path.join(ROOT, "tests", "c_inflate_host.cpp"),
                           "-o", exe])
    return exe


def run_host(exe, cases, tmp_path):
    src, dst = str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")
    with open(src, "wb") as fh:
        fh.write(struct.pack("<I", len(cases)))
        for _, p, isize, crc, verify in cases:
            fh.write(struct.pack("<IIII", len(p), isize, crc, verify) + p)
    done = subprocess.run([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0 and "c inflate host ok: %d cases" % len(cases) in done.stdout, done.stdout[-4000:]
    raw, at, out = open(dst, "rb").read(), 0, []
    for _ in cases:
        status, n = struct.unpack_from("<II", raw, at)
        out.append((status, raw[at + 8:at + 8 + n]))
        at += 8 + n
    assert at == len(raw)
    return out


def test_host_build_agrees_with_the_restatement(host_program, tmp_path):
    cases = all_cases()
    results = run_host(host_program, cases, tmp_path)
    seen = set()
    for (name, p, isize, crc, verify), (status, out) in zip(cases, results):
        want_out, want = R.inflate_payload(p, isize, crc if verify else None)
        assert status == want, (name, status, want)
        assert out == want_out, name                     # on a failure too: both stop at the same byte
        seen.add(status)
    assert seen >= {want for _, _, _, want in R.malformed_cases()} | {R.OK, R.CRC}, sorted(seen)


def test_the_header_needs_no_hip(tmp_path):
    """plain g++ compiles the header alone, with every warning an error"""
    src = tmp_path / "only.cpp"
    src.write_text('#include "inflate_core.hpp"\nint main() { return smh::inflate::kReasons == 15 ? 0 : 1; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I",
                           os.path.join(ROOT, "sourmash-rust_amd", "csrc"), str(src)])
