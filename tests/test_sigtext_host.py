"""The shared core of signature JSON written on the device (csrc/sigtext_core.hpp) built for the host under the address and
undefined-behaviour sanitizers and run as a child process (tests/c_sigtext_host.cpp): the serial driver's text, document
offsets and per-node md5 must equal the restatement's on the fixtures, the crafted sketches (every digit-count edge, every
padding length of the md5 message for ksize 7, 21 and 100) and 500 random indexes, and the program must end clean.  Nothing is
preloaded and no library is loaded into Python.  This is the gate in front of tests/test_gpu_sigtext.py: the kernels compile
the same source."""
import hashlib
import os
import struct
import subprocess

import pytest

import sigtext_restatement as R
from conftest import ROOT


def all_cases():
    """[(label, sketches, names, filenames, doc_starts)]"""
    fx = R.fixture_sketches()
    with_abunds = [p for p in fx if p[0]["abunds"] is not None]
    without = [p for p in fx if p[0]["abunds"] is None]
    cases = []
    for label, part in (("fixtures_abund", with_abunds), ("fixtures_plain", without)):
        if part:
            cases.append((label, [p[0] for p in part], [p[1] for p in part], [p[2] for p in part], None))
    for label, sketches, names, filenames in R.crafted_groups():
        n = len(sketches)
        cases.append((label, sketches, names, filenames, None))
        cases.append((label + "_docs", sketches, names, filenames, [0, 0, 1, 1, n, n]))
        cases.append((label + "_each", sketches, names, filenames, list(range(n + 1))))
    cases.append(("no_nodes", [], None, None, None))
    cases.append(("no_nodes_three_documents", [], None, None, [0, 0, 0, 0]))
    cases += [("random_%d" % i,) + r for i, r in enumerate(R.random_indexes(500))]
    return cases


def pack_cases(cases):
    out = [struct.pack("<I", len(cases))]
    for _, sketches, names, filenames, doc_starts in cases:
        n = len(sketches)
        has_abunds = int(bool(sketches) and sketches[0]["abunds"] is not None)
        out.append(struct.pack("<IIII", n, has_abunds, int(doc_starts is not None), len(doc_starts) - 1 if doc_starts else 0))
        if doc_starts is not None:
            out.append(struct.pack("<%dI" % len(doc_starts), *doc_starts))
        for v, sk in enumerate(sketches):
            out.append(struct.pack("<IIQQI", sk["num"], sk["ksize"], sk["seed"], sk["max_hash"], R.MOLECULES.index(sk["molecule"])))
            for strings in (names, filenames):
                s = None if strings is None else strings[v]
                raw = b"" if s is None else s.encode("utf-8")
                out.append(struct.pack("<i", -1 if s is None else len(raw)) + raw)
            out.append(struct.pack("<Q", len(sk["mins"])) + struct.pack("<%dQ" % len(sk["mins"]), *sk["mins"]))
            if has_abunds:
                out.append(struct.pack("<%dI" % len(sk["abunds"]), *sk["abunds"]))
    return b"".join(out)


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sigtext_host") / "c_sigtext_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "sourmash-rust_amd", "csrc"), os.path.join(ROOT, "tests", "c_sigtext_host.cpp"),
                           "-o", exe])
    return exe


def test_host_build_agrees_with_the_restatement(host_program, tmp_path):
    cases = all_cases()
    src, dst = str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")
    with open(src, "wb") as fh:
        fh.write(pack_cases(cases))
    done = subprocess.run([host_program, src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0 and "c sigtext host ok: %d cases" % len(cases) in done.stdout, done.stdout[-4000:]
    raw, at = open(dst, "rb").read(), 0
    pad_lengths = set()
    for label, sketches, names, filenames, doc_starts in cases:
        (length,) = struct.unpack_from("<Q", raw, at)
        at += 8
        text = raw[at:at + length]
        at += length
        (entries,) = struct.unpack_from("<I", raw, at)
        at += 4
        offs = list(struct.unpack_from("<%dQ" % entries, raw, at))
        at += 8 * entries
        md5 = raw[at:at + 16 * len(sketches)]
        at += 16 * len(sketches)
        want, want_offs = R.text(sketches, names, filenames, doc_starts)
        assert text == want, label
        assert offs == want_offs, label
        for v, sk in enumerate(sketches):
            message = (str(sk["ksize"]) + "".join(str(h) for h in sk["mins"])).encode()
            assert md5[16 * v:16 * v + 16] == hashlib.md5(message).digest(), (label, v)
            if label.startswith("pad_k"):
                pad_lengths.add((sk["ksize"], len(message)))
    assert at == len(raw)
    assert {L for _, L in pad_lengths} == set(R.PAD_LENGTHS) and {k for k, _ in pad_lengths} == {7, 21, 100}


def test_the_header_needs_no_hip(tmp_path):
    """plain g++ compiles the header alone, with every warning an error"""
    src = tmp_path / "only.cpp"
    src.write_text('#include "sigtext_core.hpp"\nint main() { return smh::sigtext::digits_u64(10) == 2 ? 0 : 1; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I",
                           os.path.join(ROOT, "sourmash-rust_amd", "csrc"), str(src)])
