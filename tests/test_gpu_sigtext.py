"""Signature JSON written on the device: the text and the md5s of a resident index against the restatement
(tests/sigtext_restatement.py: plain str() and hashlib), against the md5sum strings sourmash wrote into the fixtures, and, for
every constructor of an index, against the host writer over idx.sketches().  T is values_per_tile and S md5_values_per_step of
smh_sigtext_geometry: node sizes sit on both sides of them."""
import ctypes as C
import hashlib
import random

import numpy as np
import pytest

import sigtext_restatement as R

pytestmark = pytest.mark.gpu


def geometry(pkg):
    t, th, s = C.c_uint32(), C.c_uint32(), C.c_uint32()
    pkg.lib().smh_sigtext_geometry(C.byref(t), C.byref(th), C.byref(s))
    return t.value, s.value


def count(pkg, name):
    ms, k = C.c_double(), C.c_uint64()
    pkg.lib().smh_profile_get(name.encode(), C.byref(ms), C.byref(k))
    return k.value


def lib_sketch(pkg, sk):
    mh = pkg.KmerMinHash(sk["num"], sk["ksize"], False, sk["seed"], sk["max_hash"], sk["abunds"] is not None,
                         alphabet=None if sk["molecule"] == "DNA" else sk["molecule"])
    if len(sk["mins"]) > 4096 and sk["abunds"] is None:
        mh.add_many(np.array(sk["mins"], dtype=np.uint64))
        return mh
    for h in sk["mins"]:
        mh.mins_push(h)
    for a in sk["abunds"] or ():
        mh.abunds_push(a)
    return mh


def index_of(pkg, sketches):
    return pkg.index.ResidentIndex([lib_sketch(pkg, sk) for sk in sketches])


def values(rng, m, digits=None):
    out = set()
    while len(out) < m:
        d = digits or rng.randrange(1, 21)
        out.add(rng.randrange(10 ** (d - 1) if d > 1 else 0, 10 ** d) % 2 ** 64)
    return sorted(out)


def tile_edge_sketches(pkg, shift, with_abunds, seed=5):
    """nodes of 0, 1, T - 1, T, T + 1, 3T + 5 values, 70 empty nodes in a row, then 1; `shift` values more in node 0"""
    T, _ = geometry(pkg)
    rng = random.Random(seed)
    sizes = [0 + shift, 1, T - 1, T, T + 1, 3 * T + 5] + [0] * 70 + [1]
    out = []
    for m in sizes:
        mins = values(rng, m)
        abunds = [rng.randrange(10 ** rng.randrange(1, 11)) % 2 ** 32 for _ in mins] if with_abunds else None
        out.append(R.sketch(mins, abunds, ksize=rng.choice((7, 21, 100))))
    return out


def doc_shapes(n):
    return (None, list(range(n + 1)), [0, 0, 0, 2, 2, 5, n, n, n])


def check_text(idx, sketches, names=None, filenames=None, shapes=None):
    n = len(sketches)
    for doc_starts in shapes or doc_shapes(n):
        want, offs = R.text(sketches, names, filenames, doc_starts)
        t = idx.sigtext(names, filenames, doc_starts)
        assert len(t) == len(want)
        got = t.read()
        assert got == want, (doc_starts, next(i for i in range(len(want)) if got[i] != want[i]))
        assert t.doc_offsets.tolist() == offs
    assert idx.md5sums() == [R.md5_hex(sk["ksize"], sk["mins"]) for sk in sketches]


def test_fixtures_md5sums_and_load_back(pkg):
    from sourmash_rust_amd.signature import load_signatures_buffer, load_signatures_path
    for path in R.fixture_paths():
        idx = pkg.index.ResidentIndex.from_signatures(path)
        assert idx.md5sums() == [e.md5sum for e in idx.signatures], path
        text = idx.save_signatures()                           # names and filenames from the entries
        back, orig = load_signatures_buffer(text), load_signatures_path(path)
        assert len(back) == len(orig) >= 1
        assert all(a == b for a, b in zip(back, orig)), path
        assert [s.name for s in back] == [s.name for s in orig]


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_tile_edges_every_abundance_home_and_document_shape(pkg, shift):
    plain = tile_edge_sketches(pkg, shift, False)
    check_text(index_of(pkg, plain), plain, names=["n%d" % v if v % 3 else None for v in range(len(plain))])
    abund = tile_edge_sketches(pkg, shift, True)
    host = index_of(pkg, abund)                                # abundances on the host
    check_text(host, abund, filenames=[R.NAMES[v % len(R.NAMES)] for v in range(len(abund))])
    resident = host.filter()                                   # the same nodes, abundances resident in HBM
    assert resident.has_abundances
    check_text(resident, abund)
    text = host.save_signatures()
    again = pkg.index.ResidentIndex.from_signatures(text)      # resident too, by the other constructor
    check_text(again, abund, names=[None] * len(abund), filenames=[None] * len(abund))


def test_digit_count_edges_molecules_and_names(pkg):
    for label, sketches, names, filenames in R.crafted_groups():
        n = len(sketches)
        check_text(index_of(pkg, sketches), sketches, names, filenames, shapes=(None, list(range(n + 1))))


def test_md5_step_edges_and_a_long_node(pkg):
    _, S = geometry(pkg)
    rng = random.Random(9)
    sketches = [R.sketch(values(rng, m), ksize=k) for m, k in ((S - 1, 21), (S, 31), (S + 1, 7), (2 * S, 100), (2 * S + 1, 21))]
    sketches += [R.sketch(values(rng, S, digits=20)), R.sketch(values(rng, 10, digits=1))]
    idx = index_of(pkg, sketches)
    assert idx.md5sums() == [R.md5_hex(sk["ksize"], sk["mins"]) for sk in sketches]
    long = R.sketch([10 ** 19 + i * 40000000000000 for i in range(200000)])
    assert long["mins"][-1] < 2 ** 64 and len(str(long["mins"][0])) == 20
    one = index_of(pkg, [long])
    assert one.md5sums() == [hashlib.md5(("21" + "".join(map(str, long["mins"]))).encode()).hexdigest()]


def test_every_constructor_writes_what_its_sketches_say(pkg):
    """the text equals the host writer over idx.sketches(), whichever way the index was made"""
    from sourmash_rust_amd.signature import Signature, save_signatures
    rng = random.Random(3)

    def host_text(idx):
        sigs = []
        for mh in idx.sketches():
            s = Signature()
            s.push_mh(mh)
            sigs.append(s)
        return save_signatures(sigs).encode("utf-8")

    mixed = [R.sketch(values(rng, 40), num=0, ksize=21), R.sketch(values(rng, 30), num=50, max_hash=0, ksize=31),
             R.sketch(values(rng, 20), molecule="protein", ksize=30), R.sketch(values(rng, 10), molecule="dayhoff", ksize=33, seed=7),
             R.sketch(values(rng, 5), num=20, max_hash=0, molecule="hp", ksize=42)]
    made = {"host": index_of(pkg, mixed)}
    mx = 2 ** 64 // 4
    scaled = [R.sketch([h for h in values(rng, 300) if h <= mx], max_hash=mx) for _ in range(6)]
    base = index_of(pkg, scaled)
    made["downsample"] = base.downsample(max_hash=mx // 8)
    made["collapse"] = base.collapse([0, 0, 1, 1, 2, 2], n_groups=3)
    made["select"] = base.select([5, 0, 0, 3, 5])
    made["concat"] = pkg.index.ResidentIndex.concat([base, made["select"]])
    like = pkg.KmerMinHash(0, 21, False, 42, 2 ** 64 // 10, True)
    dna = ["".join(rng.choice("ACGT") for _ in range(3000)).encode() for _ in range(4)]
    made["from_records"] = pkg.index.ResidentIndex.from_records(dna, like, groups=[0, 1, 1, 2])
    differ = [name for name, idx in made.items() if idx.save_signatures() != host_text(idx)]
    assert not differ, "the device text and save_signatures(idx.sketches()) disagree for: %s" % differ


def test_grid_cap_and_pool_fill_change_nothing(pkg):
    sketches = tile_edge_sketches(pkg, 1, True)
    idx = index_of(pkg, sketches)
    want = R.text(sketches)[0]
    want_md5 = [R.md5_hex(sk["ksize"], sk["mins"]) for sk in sketches]
    try:
        for cap in (1, 2):
            pkg.matrix.set_grid_cap(cap)
            before = count(pkg, "grid_capped")
            assert idx.save_signatures() == want and idx.md5sums() == want_md5
            assert count(pkg, "grid_capped") > before, cap
    finally:
        pkg.matrix.set_grid_cap(0)
    try:
        for byte in (0x00, 0xFF):
            pkg.matrix.set_pool_fill(byte)
            assert idx.save_signatures() == want and idx.md5sums() == want_md5
    finally:
        pkg.matrix.set_pool_fill(-1)
    assert pkg.matrix.grid_cap() == 0


def test_round_trip_through_the_device_reader(pkg):
    from sourmash_rust_amd.signature import SignatureScan
    sketches = tile_edge_sketches(pkg, 2, True)
    idx = index_of(pkg, sketches)
    n = len(sketches)
    before = count(pkg, "index_sigtext")
    text, doc_offsets = idx.save_signatures(doc_starts=[0, 0, 3, n], device=True)
    assert count(pkg, "index_sigtext") == before + 1
    assert text.is_cuda and text.numel() == int(doc_offsets[-1]) and len(doc_offsets) == 4
    scan = SignatureScan.parse(text, doc_offsets)
    back = pkg.index.ResidentIndex.from_signatures(scan)
    for a, b in zip(idx.read(), back.read()):
        assert np.array_equal(a, b)
    assert [e.md5sum for e in back.signatures] == idx.md5sums() == back.md5sums()


def test_text_past_4_gib(pkg):
    import torch
    one = R.sketch([10 ** 19 + i * 8000000000000 for i in range(2 ** 20)])
    assert one["mins"][-1] < 2 ** 64
    sig_len = len(R.signature_text(one, None, None))
    m = (2 ** 32 + 2 ** 26) // (sig_len + 1) + 2
    idx = index_of(pkg, [one]).select([0] * m)
    t = idx.sigtext()
    total = len(t)
    assert total == R.text_len([one] * m) == 2 + m * sig_len + (m - 1) and total > 2 ** 32 + 2 ** 26
    view = t.view()
    first = view[1:1 + sig_len]
    for j in range(1, m):
        at = 1 + j * (sig_len + 1)
        assert torch.equal(view[at:at + sig_len], first), j
    want = R.signature_text(one, None, None).encode()
    assert t.read(1, sig_len) == want
    assert t.read(1 + (m - 1) * (sig_len + 1), sig_len + 1) == want + b"]"
    assert t.read(0, 1) == b"[" and t.read(sig_len + 1, 1) == b","
    md5 = idx.md5sums()
    assert md5 == [R.md5_hex(21, one["mins"])] * m
    del view, first
    del t


def read_hashes(idx):
    """offsets and hashes through smh_index_read (the abundances of an index that holds one of 2^32 are refused there too)"""
    from sourmash_rust_amd._lib import u64p
    off = np.zeros(len(idx) + 1, dtype=np.uint64)
    assert idx._L.smh_index_read(idx._h, off.ctypes.data_as(u64p), None, None) == 0
    hashes = np.zeros(max(int(off[-1]), 1), dtype=np.uint64)
    assert idx._L.smh_index_read(idx._h, None, hashes.ctypes.data_as(u64p), None) == 0
    return off, hashes


def test_refusals_leave_the_index_as_it_was(pkg):
    sketches = [R.sketch([1, 2, 3], [1, 1, 1]), R.sketch([4, 5], [7, 2 ** 32])]
    idx = index_of(pkg, sketches)
    before = read_hashes(idx)
    with pytest.raises(pkg.SourmashError) as ei:
        idx.save_signatures()
    assert ei.value.code == 3 and ei.value.message.startswith("sigtext:") and "node 1" in ei.value.message
    ok = index_of(pkg, [R.sketch([1, 2, 3]), R.sketch([4, 5])])
    for bad, entry in (([1, 2], "doc_starts[0]"), ([0, 1], "doc_starts[1]"), ([0, 2, 1, 2], "doc_starts[2]")):
        with pytest.raises(pkg.SourmashError) as ei:
            ok.save_signatures(doc_starts=bad)
        assert ei.value.code == 3 and ei.value.message.startswith("sigtext:") and entry in ei.value.message, bad
    for a, b in zip(before, read_hashes(idx)):
        assert np.array_equal(a, b)
    assert ok.save_signatures() == R.text([R.sketch([1, 2, 3]), R.sketch([4, 5])])[0]
    assert idx.md5sums() == [R.md5_hex(21, [1, 2, 3]), R.md5_hex(21, [4, 5])]


def test_an_index_without_nodes(pkg):
    idx = pkg.index.ResidentIndex([])
    assert idx.save_signatures() == b"[]" and idx.md5sums() == []
    assert idx.save_signatures(doc_starts=[0, 0, 0]) == b"[][]"
    text, offs = idx.save_signatures(device=True)
    assert text.numel() == 2 and offs.tolist() == [0, 2]
