"""The shared core of the signature scan and the JSON parser with holes built for the host under the address and
undefined-behaviour sanitizers and run as a child process (tests/c_sigscan_host.cpp) on the fixtures, every crafted document
and 2 000 byte-level mutants: the serial driver must give the restatement's skeleton, spans and values, the parse with holes
must accept and refuse each document as the plain parse of the host loader does (or refuse it as a float split in two), both
must read the same sketches, and the program must end clean.  Nothing is preloaded and no library is loaded into Python.
This is the gate in front of tests/test_gpu_sigscan.py: the kernels run the same source."""
import os
import struct
import subprocess

import pytest

import sigscan_restatement as R
from conftest import ROOT


def all_cases():
    """[(name, text, doc_offsets)]"""
    cases = [("fixture_%d" % i, t, [0, len(t)]) for i, t in enumerate(R.fixture_texts())]
    cases += [(name, t, [0, len(t)]) for name, t in R.crafted_documents()]
    texts = R.fixture_texts()
    offs = [0]
    for t in texts:
        offs.append(offs[-1] + len(t))
    cases.append(("fixtures_together", b"".join(texts), offs))
    good = R.document([R.signature_json([R.sketch_json([1, 2, 3], [1, 1, 1])])])
    cases.append(("no_documents", b"", [0]))
    cases.append(("empty_between", good + good, [0, len(good), len(good), 2 * len(good)]))
    cases.append(("second_fails", good + good[:-1], [0, len(good), 2 * len(good) - 1]))
    cases.append(("array_over_the_boundary", good + good, [0, len(good) + 200, 2 * len(good)]))
    cases.append(("boundary_in_a_span", good + good, [0, good.index(b"[1,2,3]") + 3, 2 * len(good)]))
    cases.append(("blank_led", good + b" \n" + good, [0, len(good), 2 * len(good) + 2]))
    cases += [("mutant_%d" % i, t, [0, len(t)]) for i, t in enumerate(R.mutants(2000))]
    return cases


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sigscan_host") / "c_sigscan_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "sourmash-rust_amd", "csrc"), os.path.join(ROOT, "tests", "c_sigscan_host.cpp"),
                           "-o", exe])
    return exe


def run_host(exe, cases, tmp_path):
    src, dst = str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")
    with open(src, "wb") as fh:
        fh.write(struct.pack("<I", len(cases)))
        for _, text, offs in cases:
            fh.write(struct.pack("<I", len(offs) - 1) + struct.pack("<%dQ" % len(offs), *offs) + struct.pack("<Q", len(text)) + text)
    done = subprocess.run([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0 and "c sigscan host ok: %d cases" % len(cases) in done.stdout, done.stdout[-4000:]
    raw, at, out = open(dst, "rb").read(), 0, []
    for _ in cases:
        vh, dh, vp, dp, agree, n_sketches, sl = struct.unpack_from("<IIIIIIQ", raw, at)
        at += 32
        skeleton = raw[at:at + sl]
        at += sl
        (ns,) = struct.unpack_from("<Q", raw, at)
        at += 8
        spans = []
        for _ in range(ns):
            start, end, first, ntok, bad, status = struct.unpack_from("<QQQQQI", raw, at)
            at += 44
            spans.append({"start": start, "end": end, "first_token": first, "n_tokens": ntok, "status": status, "bad_off": bad})
        (nv,) = struct.unpack_from("<Q", raw, at)
        at += 8
        values = list(struct.unpack_from("<%dQ" % nv, raw, at))
        at += 8 * nv
        out.append({"holes": (vh, dh), "plain": (vp, dp), "agree": agree, "sketches": n_sketches, "skeleton": skeleton, "spans": spans,
                    "values": values})
    assert at == len(raw)
    return out


def test_host_build_agrees_with_the_restatement_and_the_plain_parse(host_program, tmp_path):
    cases = all_cases()
    results = run_host(host_program, cases, tmp_path)
    verdicts, statuses = {}, set()
    for (name, text, offs), got in zip(cases, results):
        skeleton, spans, values = R.scan(text)
        assert got["skeleton"] == skeleton, name
        assert got["spans"] == spans, name
        assert got["values"] == values, name
        statuses |= {s["status"] for s in spans}
        if got["holes"][0] == 2:                                  # the one deviation: the plain parse may say either
            assert b"." in text or b"e" in text or b"E" in text, name
        else:
            assert got["holes"] == got["plain"], (name, got["holes"], got["plain"])
        assert got["agree"] == 1, name
        verdicts[name] = got["holes"][0]
        if name.startswith("fixture"):
            assert got["holes"][0] == 0 and got["sketches"] >= 1, name
    assert statuses == {R.CLOSED, R.OPEN, R.OVERFLOW, R.BAD_SYNTAX}
    # the statuses where they decide: BAD_SYNTAX anywhere, OVERFLOW only in an array read as u64, OPEN by what follows
    for k, (span, status) in enumerate(R.STATUS_SPANS):
        floats = span in (b"[1.5]", b"[1e3]")
        nested = span == b"[1,[2],3]"
        want_ignored = 2 if floats else 1 if status == R.BAD_SYNTAX or span == b"[1,]" else 0
        assert verdicts["ignored_%d" % k] == want_ignored, span[:40]
        want_mins = 2 if floats else 0 if status == R.CLOSED and not nested else 1
        assert verdicts["mins_%d" % k] == want_mins, span[:40]
        assert verdicts["abund_%d" % k] == want_mins, span[:40]
    accepted = {"empty_document", "blank_document", "no_sketches", "two_signatures", "null_abundances", "abund_other_length", "num_sketch", "q9",
                "hp", "version_int", "bracket_in_key", "nested_ignored", "objects_in_array", "deep_array", "deep_empty", "true_after_comma",
                "duplicate_mins", "fixtures_together", "no_documents", "blank_led"} | {"decoy_%d" % k for k in range(len(R.DECOY_NAMES))}
    refused = {"empty_text", "not_an_array", "number_document", "numbers_document", "trailing", "unclosed", "unclosed_mins", "cut_in_string",
               "sketch_is_number", "sketch_is_number_2", "missing_mins", "mins_is_string", "mins_nested", "mins_with_string", "mins_negative",
               "mins_true", "version_bad", "backslash_outside", "too_deep_array", "float_after_blank", "minus_glued", "letters_glued",
               "seed_overflow", "ksize_big", "empty_between", "second_fails", "array_over_the_boundary", "boundary_in_a_span"}
    assert not [n for n in accepted if verdicts[n] != 0] and not [n for n in refused if verdicts[n] != 1]
    assert verdicts["mins_float"] == 2 and verdicts["float_exp"] == 2
    mutants = [v for n, v in verdicts.items() if n.startswith("mutant_")]
    assert min(mutants.count(0), mutants.count(1)) > 100 and len(mutants) == 2000      # the mutants reach both sides


def test_the_headers_need_no_hip(tmp_path):
    """plain g++ compiles the two headers alone, with every warning an error"""
    src = tmp_path / "only.cpp"
    src.write_text('#include "sigjson.hpp"\nint main() { return smh::sigscan::kStates == 8 ? 0 : 1; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I",
                           os.path.join(ROOT, "sourmash-rust_amd", "csrc"), str(src)])
