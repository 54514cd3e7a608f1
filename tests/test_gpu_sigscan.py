"""Signature JSON read on the device: the spans and values against the restatement
(tests/sigscan_restatement.py), the entries and the index against the host route, ResidentIndex(load_signatures_buffer(...)).
No expected value here comes from the code under test.  T is the tile of the scan kernels (smh_sigscan_geometry); the tiles
are cut on 16-byte boundaries of the ADDRESS, so a text at alignment a has its tile edges at text offsets k T - a."""
import ctypes as C
import gzip
import json

import numpy as np
import pytest

import inflate_restatement as IR
import sigscan_restatement as R
import stream_order as SO

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SERDE, MSG = 100004, 3


@pytest.fixture(scope="module")
def sg(pkg):
    from sourmash_rust_amd import signature
    return signature


@pytest.fixture(scope="module")
def T(pkg):
    tile, threads = C.c_uint32(), C.c_uint32()
    pkg.lib().smh_sigscan_geometry(C.byref(tile), C.byref(threads))
    assert tile.value == 16 * threads.value
    return tile.value


def at_alignment(text, align):
    """the text in device memory with data_ptr() % 16 == align"""
    buf = torch.zeros(len(text) + 32, dtype=torch.uint8, device="cuda")
    view = buf[align:align + len(text)]
    if text:
        view.copy_(torch.frombuffer(bytearray(text), dtype=torch.uint8))
    assert not text or view.data_ptr() % 16 == align
    return view


def offsets_of(docs):
    return np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.uint64)


def check_scan(sg, text, offs=None, align=None, want=None):
    """parses `text` (host bytes, or on the device at an alignment) and holds spans and values against the restatement"""
    scan = sg.SignatureScan.parse(text if align is None else at_alignment(text, align), offs)
    _, spans, values = want if want is not None else R.scan(text)
    assert scan.n_spans == len(spans) and scan.n_tokens == len(values)
    assert scan.spans() == spans
    got = scan.values().cpu().numpy().view(np.uint64)
    assert np.array_equal(got, np.array(values, dtype=np.uint64))
    return scan


def host_route(sg, docs, ksize=0, moltype=None):
    """(signatures, sketches) of the host loader over every document in order"""
    sigs = [s for d in docs for s in sg.load_signatures_buffer(d, ksize, moltype)]
    return sigs, [s.first_mh() for s in sigs]


def entries_equal_host(scan_entries, sigs, mhs, docs_json=None):
    assert len(scan_entries) == len(sigs)
    for e, s, mh in zip(scan_entries, sigs, mhs):
        assert (e.name or "") == s.name and (e.filename or "") == s.filename and e.license == s.license
        assert (e.num, e.ksize, e.seed, e.max_hash, e.molecule) == (mh.num, mh.ksize, mh.seed, mh.max_hash, mh.molecule)
        assert e.n_mins == len(mh) and e.has_abundances == bool(mh.track_abundance)


def indexes_equal(a, b):
    (oa, ha, aa), (ob, hb, ab) = a.read(), b.read()
    assert np.array_equal(oa, ob) and np.array_equal(ha, hb)
    assert a.has_abundances == b.has_abundances and (aa is None) == (ab is None)
    if aa is not None:
        assert np.array_equal(aa, ab)
    assert a.max_hash_range == b.max_hash_range and len(a) == len(b)


def raises_code(fn):
    from sourmash_rust_amd import SourmashError
    try:
        fn()
    except SourmashError as e:
        return e.code, e.message
    return 0, ""


# ------------------------------------------------------------------------------------------------------- fixture documents
def test_fixture_documents_in_one_call(pkg, sg):
    docs = R.fixture_texts()
    text, offs = b"".join(docs), offsets_of(docs)
    scan = check_scan(sg, text, offs)
    sigs, mhs = host_route(sg, docs)
    assert len(scan) == 11
    entries_equal_host(scan.entries, sigs, mhs)
    # document, signature and sketch of every entry, the md5sum as written: from Python's json
    want = [(d, i, k, sk["md5sum"]) for d, doc in enumerate(docs) for i, sig in enumerate(json.loads(doc)) for k, sk in enumerate(sig["signatures"])]
    assert [(e.document, e.signature, e.sketch, e.md5sum) for e in scan.entries] == want
    host = pkg.index.ResidentIndex(mhs)
    dev = pkg.index.ResidentIndex.from_signatures(scan)
    indexes_equal(dev, host)
    assert [t[:5] for t in dev._node_templates] == [(m.num, m.ksize, m.molecule, m.seed, m.max_hash) for m in mhs]
    assert [e.name or "" for e in dev.signatures] == [s.name for s in sigs]
    same = [i for i, m in enumerate(mhs) if (m.ksize, m.molecule) == (31, "DNA")]
    assert len(same) == 7
    d31, h31 = pkg.index.ResidentIndex.from_signatures(scan, ids=same), pkg.index.ResidentIndex([mhs[i] for i in same])
    indexes_equal(d31, h31)
    for q in (mhs[same[0]], mhs[same[3]]):
        assert d31.find(q, 0.0) == h31.find(q, 0.0) and d31.find(q, 0.05, containment=True) == h31.find(q, 0.05, containment=True)
        assert q is not mhs[same[0]] or len(d31.find(q, 0.0)) >= 1
    assert np.array_equal(d31.compare(d31)["jaccard"], h31.compare(h31)["jaccard"])
    # the search of a batch: scaled sketches (a synthetic collection, both routes)
    sk = [R.sketch_json(sorted(set(range(i, 4000, 3 + i % 5))), max_hash=R.U64_MAX // 2) for i in range(12)]
    doc = R.document([R.signature_json([s], name=b'"s%d"' % i) for i, s in enumerate(sk)])
    sigs2, mhs2 = host_route(sg, [doc])
    host2, dev2 = pkg.index.ResidentIndex(mhs2), pkg.index.ResidentIndex.from_signatures(doc)
    indexes_equal(dev2, host2)
    a, b = dev2.search_many(mhs2[:5], 0.1), host2.search_many(mhs2[:5], 0.1)
    assert len(a) > 5 and np.array_equal(a.offsets, b.offsets) and np.array_equal(a.node, b.node) and np.array_equal(a.common, b.common)
    assert [m.mins for m in dev2.sketches()] == [m.mins for m in mhs2]
    both = pkg.index.ResidentIndex.concat([dev2, dev2.select([3, 1])])
    assert len(both) == 14 and both.sketches()[13].mins == mhs2[1].mins


# --------------------------------------------------------------------------------------------------------- sliding features
# A text at alignment a has its tile edges at text offsets k T - a, so a feature at document offset k T + ph stands at ph + a
# against its own edge: with ph = -35 .. +20 every alignment 0 .. 15 sees each phase -20 .. +20 (asserted below).
PHASES = list(range(-35, 21))
assert all({ph + a for ph in PHASES} >= set(range(-20, 21)) for a in range(16))


def sliding_text(T, feature):
    """Documents of exactly 3 T bytes, one per phase: the feature's byte stands at offset T + phase of its document (2 T + phase when
    what stands in front of it is longer than a tile).  Padding
    is blanks where JSON allows them: `pad1` in front of `mid` (between two tokens, or inside an array), the rest behind the
    document's last bracket."""
    tail_numbers = b",".join(b"%d" % (10 ** 6 + 7 * i) for i in range(T // 6))           # more than a tile of digits
    abund = b',"abundances":[' + b",".join(b"1" for _ in range(T // 6)) + b"]"
    head = b'[{"class":"sourmash_signature","email":"","hash_function":"0.murmur64","filename":"f","name":'
    sketch_open = b',"license":"CC0","signatures":[{"num":0,"ksize":21,"seed":42,"max_hash":18446744073709551615,"md5sum":"m","molecule":"DNA"'
    close = b"}]}]"
    kind, arg = feature
    if kind == "open":
        pre, mid, foff = head + b'"n"' + sketch_open + b',"mins":', b"[" + tail_numbers + b"]" + abund + close, 0
    elif kind == "close":
        pre, mid, foff = head + b'"n"' + sketch_open + abund + b',"mins":[' + tail_numbers + b",", b"9999999999]" + close, 10
    elif kind == "quote":
        pre, mid = b"[", head[1:] + b'"abc[1,2"' + sketch_open + b',"mins":[' + tail_numbers + b"]" + abund + close
        foff = len(head) - 1 + 8
    elif kind == "backslashes":
        run = b"\\" * arg
        name = b'"x' + run + (b'"[7,8] y"' if arg % 2 else b'"')
        extra = b"" if arg % 2 else b',"k":[7,8]'
        pre, mid = b"[", head[1:] + name + extra + sketch_open + b',"mins":[' + tail_numbers + b"]" + abund + close
        foff = len(head) - 1 + 2 + arg
    elif kind == "max_token":
        pre, mid, foff = head + b'"n"' + sketch_open + abund + b',"mins":[' + tail_numbers + b",", b"18446744073709551615]" + close, 0
    else:
        assert kind == "comma"
        pre, mid, foff = head + b'"n"' + sketch_open + abund + b',"mins":[' + tail_numbers, b" \t, \n9999999999]" + close, 2
    edge = T if len(pre) + foff <= T + PHASES[0] else 2 * T          # the first or the second edge inside the document
    docs = []
    for ph in PHASES:
        pad1 = edge + ph - len(pre) - foff
        assert pad1 >= 0, (feature, pad1)
        body = pre + b" " * pad1 + mid
        assert body[edge + ph] == mid[foff] and len(body) <= 3 * T, (feature, len(body))
        docs.append(body + b"\n" * (3 * T - len(body)))
    return docs


FEATURES = [("open", 0), ("close", 0), ("quote", 0), ("backslashes", 1), ("backslashes", 2), ("backslashes", 3), ("backslashes", 4),
            ("max_token", 0), ("comma", 0)]


@pytest.mark.parametrize("feature", FEATURES, ids=lambda f: "%s%s" % (f[0], f[1] or ""))
def test_a_feature_slid_over_a_tile_edge_at_every_alignment(pkg, sg, T, feature):
    docs = sliding_text(T, feature)
    text, offs = b"".join(docs), offsets_of(docs)
    want = R.scan(text)
    sigs, mhs = host_route(sg, docs[:2])
    for align in range(16):
        scan = check_scan(sg, text, offs, align=align, want=want)
        assert len(scan) == len(docs)
        entries_equal_host(scan.entries[:2], sigs, mhs)
        assert {e.n_mins for e in scan.entries} == {len(mhs[0])} and {e.name for e in scan.entries} == {sigs[0].name}
    idx = pkg.index.ResidentIndex.from_signatures(scan, ids=[0, len(docs) - 1])
    indexes_equal(idx, pkg.index.ResidentIndex([mhs[0], mhs[0]]))


# -------------------------------------------------------------------------------------------------- decoy names, statuses
def test_decoy_names(pkg, sg):
    docs = [t for name, t in R.crafted_documents() if name.startswith("decoy_")]
    assert len(docs) == len(R.DECOY_NAMES)
    scan = check_scan(sg, b"".join(docs), offsets_of(docs), align=5)
    sigs, mhs = host_route(sg, docs)
    entries_equal_host(scan.entries, sigs, mhs)
    assert [e.name for e in scan.entries] == [json.loads(n) for n in R.DECOY_NAMES] == [e.filename for e in scan.entries]
    indexes_equal(pkg.index.ResidentIndex.from_signatures(scan), pkg.index.ResidentIndex(mhs))


def test_every_crafted_document_is_accepted_or_refused_as_the_host_loader_does(pkg, sg):
    seen = set()
    for name, text in R.crafted_documents():
        host_code, _ = raises_code(lambda: sg.load_signatures_buffer(text))
        code, message = raises_code(lambda: check_scan(sg, text, align=3))
        if code == MSG:
            assert "load_signatures" in message and message.startswith("signatures: document 0, byte "), (name, message)
            assert b"." in text or b"e" in text or b"E" in text, name
        else:
            assert code == host_code and code in (0, SERDE), (name, code, host_code, message)
            assert code == 0 or message.startswith("document 0, byte "), (name, message)
        seen.add((name.split("_")[0], code))
    assert {("mins", 0), ("mins", SERDE), ("mins", MSG), ("ignored", 0), ("ignored", SERDE), ("ignored", MSG), ("abund", SERDE)} <= seen
    # the statuses themselves, where they decide
    texts = dict(R.status_documents())
    for k, (span, status) in enumerate(R.STATUS_SPANS):
        floats = span in (b"[1.5]", b"[1e3]")
        code_ignored, msg_ignored = raises_code(lambda: sg.SignatureScan.parse(texts["ignored_%d" % k]))
        code_mins, msg_mins = raises_code(lambda: sg.SignatureScan.parse(texts["mins_%d" % k]))
        if status == R.BAD_SYNTAX:                  # the device's lowest offending byte is the one the restatement names
            for text, message in ((texts["ignored_%d" % k], msg_ignored), (texts["mins_%d" % k], msg_mins)):
                bad = [s["bad_off"] for s in R.scan(text)[1] if s["status"] == R.BAD_SYNTAX]
                assert len(bad) == 1 and message.startswith("document 0, byte %d: " % bad[0]), (span[:40], bad, message)
        assert code_ignored == (MSG if floats else SERDE if status == R.BAD_SYNTAX or span == b"[1,]" else 0), span[:40]
        assert code_mins == (MSG if floats else 0 if status == R.CLOSED else SERDE), span[:40]
    # the lowest failing document decides, and its own byte is named
    good = R.document([R.signature_json([R.sketch_json([1, 2, 3])])])
    bad = good.replace(b"[1,2,3]", b"[1,,3]")
    code, message = raises_code(lambda: sg.SignatureScan.parse(good + bad + good[:-1], offsets_of([good, bad, good[:-1]])))
    assert code == SERDE and message.startswith("document 1, byte %d: " % (bad.index(b"[1,,3]") + 3)), message


# ------------------------------------------------------------------------------------------------------------- extents
def small_documents(n):
    rng = np.random.RandomState(5)
    docs = []
    for i in range(n):
        m = sorted(set(int(v) for v in rng.randint(1, 1 << 40, size=1 + i % 23)))
        sk = [R.sketch_json(m, [1 + (j + i) % 7 for j in range(len(m))], ksize=21 + 10 * (i % 2))]
        if i % 4 == 0:
            sk.append(R.sketch_json(m[:1 + len(m) // 2], [3] * (1 + len(m) // 2), ksize=31, molecule="protein"))
        docs.append(R.document([R.signature_json(sk, name=b'"doc %d"' % i)]))
    return docs


@pytest.mark.parametrize("fill", [-1, 0xA5])
@pytest.mark.parametrize("cap", [0, 1, 3])
def test_document_counts_under_grid_caps_and_pool_fill(pkg, sg, cap, fill):
    L = pkg.lib()
    docs = small_documents(300)
    L.smh_set_grid_cap(cap)
    L.smh_set_pool_fill(fill)
    try:
        for n in (0, 1, 300):
            part = docs[:n]
            scan = check_scan(sg, b"".join(part), offsets_of(part), align=n % 16)
            sigs, mhs = host_route(sg, part)
            entries_equal_host(scan.entries, sigs, mhs)
            indexes_equal(pkg.index.ResidentIndex.from_signatures(scan), pkg.index.ResidentIndex(mhs))
    finally:
        L.smh_set_grid_cap(0)
        L.smh_set_pool_fill(-1)


def test_one_array_across_many_tiles_and_the_empty_cases(pkg, sg, T):
    m = [3 + 5 * i for i in range(2 * T)]                       # far more than three tiles of digits
    doc = R.document([R.signature_json([R.sketch_json(m, max_hash=R.U64_MAX)])])
    assert len(doc) > 5 * T
    for align in (0, 9):
        scan = check_scan(sg, doc, align=align)
        assert [e.n_mins for e in scan.entries] == [len(m)]
    _, mhs = host_route(sg, [doc])
    indexes_equal(pkg.index.ResidentIndex.from_signatures(doc), pkg.index.ResidentIndex(mhs))
    # a document `[]`, a signature without sketches, no documents at all, an empty text as a document
    assert len(check_scan(sg, b"[]")) == 0 and len(check_scan(sg, b"[]", align=1)) == 0
    assert len(check_scan(sg, R.document([R.signature_json([])]))) == 0
    assert len(pkg.index.ResidentIndex.from_signatures(b"[]")) == 0
    none = sg.SignatureScan.parse(b"", [0])
    assert (len(none), none.n_spans, none.n_tokens) == (0, 0, 0) and len(pkg.index.ResidentIndex.from_signatures(none)) == 0
    assert len(sg.SignatureScan.parse(torch.empty(0, dtype=torch.uint8, device="cuda"), [0])) == 0
    code, message = raises_code(lambda: sg.SignatureScan.parse(b""))
    assert code == SERDE and message.startswith("document 0, byte 0: ")
    # the documents tile the text: bytes in front of the first or behind the last one are refused, they are not skipped
    assert raises_code(lambda: sg.SignatureScan.parse(b"[]", [0, 5]))[0] == MSG
    assert raises_code(lambda: sg.SignatureScan.parse(b'"[]', [1, 3]))[0] == MSG and raises_code(lambda: sg.SignatureScan.parse(b"[] ", [0, 2]))[0] == MSG
    assert raises_code(lambda: sg.SignatureScan.parse(b"[]", [2]))[0] == MSG
    assert raises_code(lambda: sg.SignatureScan.parse(b"[][]", [0, 3, 2]))[0] == MSG


# ----------------------------------------------------------------------------------------------------------- abundances
def test_abundances_on_all_on_some_null_and_of_another_length(pkg, sg):
    a, b, c = [2, 5, 9, 11], [1, 5, 11, 40, 41], [5, 9]
    cases = {
        "all": [R.sketch_json(a, [1, 2, 3, 4]), R.sketch_json(b, [9, 8, 7, 6, 5]), R.sketch_json(c, [1, 1])],
        "some": [R.sketch_json(a, [1, 2, 3, 4]), R.sketch_json(b), R.sketch_json(c, [1, 1])],
        "null": [R.sketch_json(a, [1, 2, 3, 4]), R.sketch_json(b, "null"), R.sketch_json(c, [1, 1])],
        "other_length": [R.sketch_json(a, [1, 2, 3, 4]), R.sketch_json(b, [9, 8, 7]), R.sketch_json(c, [1, 1])],
        "empty_arrays": [R.sketch_json([], []), R.sketch_json(c, [4, 4])],
    }
    for name, sketches in cases.items():
        doc = R.document([R.signature_json(sketches[:2]), R.signature_json(sketches[2:])])
        sigs, mhs = host_route(sg, [doc])
        host, dev = pkg.index.ResidentIndex(mhs), pkg.index.ResidentIndex.from_signatures(doc)
        assert dev.has_abundances == (name in ("all", "empty_arrays")), name
        indexes_equal(dev, host)
        if dev.has_abundances:
            assert np.array_equal(dev.norms2(), host.norms2())
            q = mhs[-1]
            x, y = dev.angular(q), host.angular(q)
            assert np.array_equal(x.dot, y.dot) and np.array_equal(x.angular, y.angular)


def test_one_abundance_of_two_to_the_32(pkg, sg):
    from sourmash_rust_amd import SourmashError
    big = R.sketch_json([4, 8, 15], [1, 1 << 32, 2])
    doc = R.document([R.signature_json([R.sketch_json([4, 8], [3, 3]), big, R.sketch_json([8, 16], [5, 1 << 40])])])
    sigs, mhs = host_route(sg, [doc])
    host, dev = pkg.index.ResidentIndex(mhs), pkg.index.ResidentIndex.from_signatures(doc)
    assert dev.has_abundances and host.has_abundances and len(dev) == 3
    # an index that holds such an abundance refuses to be read with its abundances: both name the same node
    refusals = [raises_code(idx.read) for idx in (dev, host)]
    assert refusals[0] == refusals[1] and refusals[0][0] == MSG and "node 1 " in refusals[0][1]
    assert np.array_equal(dev.sizes(), host.sizes())
    q = mhs[0]
    answers = []
    for idx in (dev, host):
        try:
            r = idx.angular(q)
            answers.append((0, r.dot.tolist(), r.angular.tolist()))
        except SourmashError as e:
            answers.append((e.code, e.message))
    assert answers[0] == answers[1]
    # without the wide nodes both answer with numbers
    d0, h0 = pkg.index.ResidentIndex.from_signatures(doc, ids=[0, 0]), pkg.index.ResidentIndex([mhs[0], mhs[0]])
    assert np.array_equal(d0.angular(q).angular, h0.angular(q).angular) and d0.angular(q).dot.tolist() == [18, 18]


# ------------------------------------------------------------------------------------------------------------- selection
def test_selection_by_ksize_and_moltype_and_by_ids(pkg, sg):
    docs = small_documents(40) + [R.document([R.signature_json([R.sketch_json([1, 7], molecule="hp"), R.sketch_json([2], molecule="dayhoff")])])]
    text, offs = b"".join(docs), offsets_of(docs)
    scan = sg.SignatureScan.parse(text, offs)
    for ksize, moltype in ((0, None), (21, None), (31, "protein"), (31, "DNA"), (0, "PROTEIN"), (0, "hp"), (21, "dayhoff"), (51, None), (0, "rna")):
        sigs, mhs = host_route(sg, docs, ksize, moltype)
        dev = pkg.index.ResidentIndex.from_signatures(scan, ksize=ksize, moltype=moltype)
        assert len(dev) == len(mhs), (ksize, moltype)
        indexes_equal(dev, pkg.index.ResidentIndex(mhs))
        assert [e.name or "" for e in dev.signatures] == [s.name for s in sigs]
    sigs, mhs = host_route(sg, docs)
    ids = list(range(len(mhs)))[::-1] + [3, 3, 0, len(mhs) - 1]
    dev = pkg.index.ResidentIndex.from_signatures(scan, ids=ids)
    indexes_equal(dev, pkg.index.ResidentIndex([mhs[i] for i in ids]))
    indexes_equal(dev, pkg.index.ResidentIndex(mhs).select(ids))
    assert raises_code(lambda: pkg.index.ResidentIndex.from_signatures(scan, ids=[0, len(mhs)]))[0] == MSG
    assert len(pkg.index.ResidentIndex.from_signatures(scan, ids=[])) == 0


def test_unsorted_and_duplicated_hashes_are_refused(pkg, sg):
    L = pkg.lib()
    ok = R.sketch_json([1, 2, 3, 4])
    doc = R.document([R.signature_json([ok, R.sketch_json([1, 5, 5, 9]), ok, R.sketch_json([9, 8, 7])])])
    scan = sg.SignatureScan.parse(doc)
    assert len(scan) == 4

    def built():
        n, ms = C.c_uint64(), C.c_double()
        L.smh_profile_get(b"index_from_signatures", C.byref(ms), C.byref(n))
        return n.value
    before = built()
    code, message = raises_code(lambda: pkg.index.ResidentIndex.from_signatures(scan))
    assert code == MSG and "node 1 " in message and "position 2" in message and "ascending" in message, message
    code, message = raises_code(lambda: pkg.index.ResidentIndex.from_signatures(scan, ids=[0, 3, 1]))
    assert code == MSG and "node 1 (sketch 3" in message and "position 1" in message, message
    assert built() == before                                        # nothing was built, nothing registered
    sound = pkg.index.ResidentIndex.from_signatures(scan, ids=[0, 2])
    assert len(sound) == 2 and built() == before + 1
    sigs, mhs = host_route(sg, [R.document([R.signature_json([ok, ok])])])
    indexes_equal(sound, pkg.index.ResidentIndex(mhs))


# ------------------------------------------------------------------------------------------------------------ past 4 GiB
def test_a_document_repeated_past_4_gib(pkg, sg):
    rng = np.random.RandomState(11)
    per = 3_300_000
    m = np.uint64(10 ** 18) + np.cumsum(rng.randint(1, 1 << 20, size=per).astype(np.uint64))     # 19 digits each
    mins_text = ("[" + ",".join(map(str, m.tolist())) + "]").encode()
    doc = R.document([R.signature_json([R.sketch_json([], max_hash=R.U64_MAX, mins_text=mins_text)])])
    doc += b" " * (-len(doc) % 4096 + 7)                         # (a length that moves every repeat against the tiles)
    assert len(doc) > 62 << 20
    reps = (1 << 32) // len(doc) + 2
    one = torch.frombuffer(bytearray(doc), dtype=torch.uint8).cuda()
    text = one.repeat(reps)
    assert text.numel() == reps * len(doc) > 1 << 32
    offs = np.arange(reps + 1, dtype=np.uint64) * np.uint64(len(doc))
    scan = sg.SignatureScan.parse(text, offs)
    del text
    assert len(scan) == reps and scan.n_tokens == reps * per and scan.n_spans == 3 * reps
    values = scan.values()
    first = torch.from_numpy(m.view(np.int64)).cuda()
    assert bool((values.view(reps, per) == first).all())
    spans = scan.spans()
    start = doc.index(mins_text) + 1
    for r in range(reps):
        mine = spans[3 * r + 2]
        assert mine == {"start": r * len(doc) + start, "end": r * len(doc) + start + len(mins_text) - 2, "first_token": r * per,
                        "n_tokens": per, "status": R.CLOSED, "bad_off": R.NONE}
        assert [(s["end"] - s["start"], s["n_tokens"]) for s in spans[3 * r:3 * r + 2]] == [(0, 0), (0, 0)]
    assert {(e.document, e.n_mins, e.max_hash) for e in scan.entries} == {(r, per, R.U64_MAX) for r in range(reps)}
    idx = pkg.index.ResidentIndex.from_signatures(scan, ids=[reps - 1])
    off, hashes, _ = idx.read()
    assert np.array_equal(hashes, m)
    del values, scan, idx


# ----------------------------------------------------------------------------------------------------- device-side BGZF
def test_a_bgzf_collection_never_leaves_the_device(pkg, sg, tmp_path):
    from sourmash_rust_amd import fastx
    docs = small_documents(60)
    sigs, mhs = host_route(sg, docs)
    host = pkg.index.ResidentIndex(mhs)
    merged = R.document([d[1:-1] for d in docs])                 # one document of every signature
    text = fastx.inflate(IR.bgzf(merged, 4000))
    assert text.is_cuda and text.numel() == len(merged)
    scan = sg.SignatureScan.parse(text)
    indexes_equal(pkg.index.ResidentIndex.from_signatures(scan), host)
    # paths: blocked gzip (inflated on the device), single-stream gzip and a plain file, each a document
    third = len(docs) // 3
    parts = [R.document([d[1:-1] for d in docs[i * third:(i + 1) * third]]) for i in range(3)]
    paths = [str(tmp_path / n) for n in ("a.sig.gz", "b.sig.gz", "c.sig")]
    open(paths[0], "wb").write(IR.bgzf(parts[0], 3000))
    open(paths[1], "wb").write(gzip.compress(parts[1]))
    open(paths[2], "wb").write(parts[2])
    from_paths = pkg.index.ResidentIndex.from_signatures(paths)
    indexes_equal(from_paths, host)
    assert [e.document for e in from_paths.signatures] == [d for d, p in enumerate(parts) for sig in json.loads(p) for _ in sig["signatures"]]
    indexes_equal(pkg.index.ResidentIndex.from_signatures(paths[2], ksize=31), pkg.index.ResidentIndex(host_route(sg, docs[2 * third:], 31)[1]))


# ---------------------------------------------------------------------------------------------------------- stream order
@pytest.mark.parametrize("which", ["caller", "null"])
def test_parse_dev_is_ordered_on_its_stream(pkg, sg, which):
    """the text is still being produced on the stream: until then the buffer holds another document of the same layout and
    length, which parses without an error to other numbers"""
    from test_gpu_stream_order import aparts
    stream = aparts(pkg)[0] if which == "caller" else torch.cuda.default_stream()
    handle = SO.handle(stream)
    assert (handle is None) == (which == "null")
    docs = [R.document([R.signature_json([R.sketch_json([10 ** 9 + base + 3 * i for i in range(20000)])])]) for base in (0, 1)]
    assert len(docs[0]) == len(docs[1]) and docs[0] != docs[1]
    true, decoy = (torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda() for d in docs)
    dst = torch.empty_like(true)
    for t in (true, decoy, dst):
        t.record_stream(stream)
    dst.copy_(true)
    torch.cuda.synchronize()
    want = np.array(R.scan(docs[0])[2], dtype=np.uint64)
    warm = sg.SignatureScan.parse(dst, stream=handle)                                    # (warm-up: the pool has its blocks)
    assert np.array_equal(warm.values().cpu().numpy().view(np.uint64), want)
    ev = SO.late(stream, dst, true, decoy)
    SO.pending(ev)
    scan = sg.SignatureScan.parse(dst, stream=handle)
    assert np.array_equal(scan.values().cpu().numpy().view(np.uint64), want)
    torch.cuda.synchronize()
