"""The restatement of signature JSON written on the device (tests/sigtext_restatement.py) against what it restates: the host
writer, signatures_save_buffer, byte for byte on the fixtures re-serialised and on crafted sketches, and the md5sum strings
sourmash itself wrote into the fixtures.  Needs no GPU.  Also the refusals the new entry points make without a device."""
import ctypes as C

import pytest

import sigtext_restatement as R


def lib_sketch(pkg, sk):
    mh = pkg.KmerMinHash(sk["num"], sk["ksize"], False, sk["seed"], sk["max_hash"], sk["abunds"] is not None,
                         alphabet=None if sk["molecule"] == "DNA" else sk["molecule"])
    for h in sk["mins"]:
        mh.mins_push(h)
    for a in sk["abunds"] or ():
        mh.abunds_push(a)
    return mh


def lib_text(pkg, sketches, names, filenames, doc_starts):
    """signatures_save_buffer of every document, one default Signature per sketch"""
    from sourmash_rust_amd.signature import Signature, save_signatures
    n = len(sketches)
    names = [None] * n if names is None else names
    filenames = [None] * n if filenames is None else filenames
    doc_starts = [0, n] if doc_starts is None else doc_starts
    out = b""
    for a, b in zip(doc_starts, doc_starts[1:]):
        sigs = []
        for v in range(a, b):
            s = Signature()
            if names[v] is not None:
                s.name = names[v]
            if filenames[v] is not None:
                s.filename = filenames[v]
            s.push_mh(lib_sketch(pkg, sketches[v]))
            sigs.append(s)
        out += save_signatures(sigs).encode("utf-8")
    return out


def test_the_crafted_inputs_cover_what_the_issue_lists():
    groups = R.crafted_groups()
    sketches = [sk for _, g, _, _ in groups for sk in g]
    hashes = {h for sk in sketches for h in sk["mins"]}
    assert {0, 9, 10, 99, 100, 10 ** 19, 10 ** 19 - 1, 2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1} <= hashes
    assert all(10 ** d in hashes and 10 ** d - 1 in hashes for d in range(1, 20))
    assert 2 ** 32 - 1 in {a for sk in sketches for a in sk["abunds"] or ()}
    assert {sk["molecule"] for sk in sketches} == set(R.MOLECULES)
    assert any(sk["num"] for sk in sketches) and any(not sk["num"] for sk in sketches) and any(not sk["mins"] for sk in sketches)
    assert {len(str(k)) + sum(len(str(h)) for h in R.hashes_for_length(L, k)) for L in R.PAD_LENGTHS for k in (7, 21, 100)
            if R.hashes_for_length(L, k) is not None} == set(R.PAD_LENGTHS)
    for L in R.PAD_LENGTHS:
        h = R.hashes_for_length(L, 7)
        assert h == sorted(set(h))


def test_restatement_equals_the_host_writer_on_crafted_sketches(pkg):
    for label, sketches, names, filenames in R.crafted_groups():
        n = len(sketches)
        for doc_starts in (None, list(range(n + 1)), [0, 0, 1, 1, n, n]):
            want, offs = R.text(sketches, names, filenames, doc_starts)
            assert lib_text(pkg, sketches, names, filenames, doc_starts) == want, (label, doc_starts)
            assert offs[-1] == len(want) == R.text_len(sketches, names, filenames, doc_starts)
    assert R.text([], None, None, None)[0] == b"[]" == lib_text(pkg, [], None, None, None)


def test_restatement_equals_the_host_writer_on_the_fixtures_reserialised(pkg):
    from sourmash_rust_amd.signature import load_signatures_path, save_signatures
    fx = R.fixture_sketches()
    at = 0
    for path in R.fixture_paths():
        loaded = load_signatures_path(path)
        part = fx[at:at + len(loaded)]
        at += len(loaded)
        want, _ = R.text([p[0] for p in part], [p[1] for p in part], [p[2] for p in part])
        assert save_signatures(loaded).encode("utf-8") == want, path
    assert at == len(fx) == 11


def test_restatement_md5_equals_what_sourmash_wrote():
    fx = R.fixture_sketches()
    assert len(fx) == 11
    lengths = set()
    for sk, _, _, md5sum in fx:
        assert R.md5_hex(sk["ksize"], sk["mins"]) == md5sum
        lengths.add((len(str(sk["ksize"])) + sum(len(str(h)) for h in sk["mins"])) % 64)
    assert 59 in lengths        # one whose padding spills into a further block


def test_new_calls_refuse_without_a_device(pkg):
    if pkg.device_available():
        pytest.skip("a GPU is present")
    L = pkg.lib()
    out = (C.c_uint8 * 16)()
    assert L.smh_index_md5(None, out) == 2
    L.sourmash_err_clear()
    assert not L.smh_index_sigtext(None, None, None, None, 0) and L.sourmash_err_get_last_code() == 2
    L.sourmash_err_clear()
    # the accessors answer for a NULL handle
    assert L.smh_sigtext_len(None) == 0 and L.smh_sigtext_documents(None) == 0 and not L.smh_sigtext_dev(None)
    L.smh_sigtext_free(None)
