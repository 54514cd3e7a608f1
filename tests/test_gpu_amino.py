"""GPU parity of amino-acid input (smh_add_protein*, k_amino_tiled / k_amino_generic) and of the dayhoff / hp alphabets on
translated input, bit-exact against tests/amino_restatement.py: hashes AND abundances.  Unless a test is about a mode,
every window is compared: max_hash = 2^64 - 1 with abundances.  Every case asserts the kernel that served it (launch
counters amino_tiled / amino_generic, or the protein arm's) and a floor on the restatement's distinct count.

The sweeps share one field of three tiles (T and R from smh_amino_geometry: window starts per workgroup tile and per lane);
its window hashes are computed once per (alphabet, W) with the oracle's murmur and a case's expectation is the subset of
windows that lie inside one record (amino_restatement.starts_inside_records, checked on the CPU against the add_word
restatement).  There is one launch geometry, so no filler records are needed to reach another."""
import ctypes as C
import itertools
import random

import numpy as np
import pytest

import amino_restatement as ar

pytestmark = pytest.mark.gpu

MAXH = (1 << 64) - 1
LETTERS = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
ALPHA_OF_W = {7: "dayhoff", 9: "protein", 10: "dayhoff", 16: "protein", 42: "hp"}
REC50 = b"MVLSPADKTNVKAAWGKVGAHAGEYGAEALERMFLSFPTTKTYFPHF*xb"
DNA96 = b"ATGGTGCTGTCTCCTGCCGACAAGACCAACGTCAAGGCCGCCTGGGGTAAGGTCGGCGCGCACGCTGGCGAGTATGGTGCGGAGGCCCTGGAGAGG"


@pytest.fixture(scope="module")
def geom(pkg):
    t, r = C.c_uint32(), C.c_uint32()
    pkg.lib().smh_amino_geometry(1 << 20, 9, C.byref(t), C.byref(r))
    return t.value, r.value


@pytest.fixture(scope="module")
def field(geom):
    """three tiles of residues: the 20 letters, a twentieth in lower case, a few '*', 'X', 'B' and NUL / 0xFF bytes"""
    n = 3 * geom[0]
    rng = np.random.default_rng(1)
    d = rng.choice(LETTERS, size=n)
    d[rng.random(n) < 0.05] |= 0x20
    for b in (ord("*"), ord("X"), ord("B"), 0x00, 0xFF):
        d[rng.integers(0, n, size=12)] = b
    return d.tobytes()


_HASHES = {}


def field_hashes(field, alpha, w):
    """hash of the window at every start of the field (one record), computed once and never changed"""
    if (alpha, w) not in _HASHES:
        h = np.asarray(ar.window_hashes(field, alpha, w), dtype=np.uint64)
        h.setflags(write=False)
        _HASHES[(alpha, w)] = h
    return _HASHES[(alpha, w)]


def on_device(data, misalign=0):
    """the bytes in HBM, `misalign` bytes past a 16-byte boundary: (tensor that owns them, pointer)"""
    import torch
    t = torch.zeros(len(data) + 64, dtype=torch.uint8, device="cuda")
    base = (-t.data_ptr()) % 16 + misalign
    t[base:base + len(data)] = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    assert (t.data_ptr() + base) % 16 == misalign % 16
    return t, t.data_ptr() + base


def new_sketch(pkg, alpha, w, num=0, max_hash=MAXH, track=True):
    return pkg.KmerMinHash(num, 3 * w, True, 42, max_hash, track, alphabet=alpha)


def assert_route(c, w, launches=None):
    tiled = w <= 64
    assert (c["amino_tiled"] >= 1) == tiled and (c["amino_generic"] >= 1) == (not tiled), c
    assert c["protein_fused"] == 0 and c["translate"] == 0 and c["hash_windows"] == 0, c
    if launches is not None:
        assert c["amino_tiled"] + c["amino_generic"] == launches, c


def check_field(pkg, alpha, w, ptr, n, offsets, h, floor):
    """the first n bytes of the field cut at `offsets`, every window kept: library == restatement"""
    mh = new_sketch(pkg, alpha, w)
    off = np.asarray(offsets, dtype=np.uint64)
    assert off[0] == 0 and off[-1] == n
    c = ar.counters(pkg, lambda: mh.add_proteins_dev(ptr, n, off))
    keep = ar.starts_inside_records(n, offsets, w)
    mins, abunds = ar.full_state(h[keep])
    assert len(mins) >= floor, len(mins)
    gm, ga = mh.mins_np(), mh.abunds_np()
    assert gm.shape == mins.shape and (gm == mins).all(), (w, list(offsets)[:8])
    assert (ga == abunds).all(), (w, list(offsets)[:8])
    assert_route(c, w, 1)


# ------------------------------------------------------------------------------------------------------------------
# known answers through the C ABI

def test_known_answers_through_the_abi(pkg):
    from test_amino_rules import KNOWN, KNOWN_TRANSLATED
    assert pkg.hash_murmur(b"bebbbbc") == 17280634798361449420 and pkg.hash_murmur(b"hhhphhp") == 15140769491848236245
    for (alpha, ksize), want in KNOWN.items():
        mh = pkg.KmerMinHash(1000, ksize, True, 42, 0, True, alphabet=alpha)
        c = ar.counters(pkg, lambda: mh.add_protein(REC50))
        assert (len(mh), int(mh.abunds_np().sum()), mh.mins[0]) == want, (alpha, ksize)
        ar.same_state(mh, ar.amino_sketch([REC50], alpha, ksize, 1000, 0))
        assert_route(c, ksize // 3)
    for alpha, want in KNOWN_TRANSLATED.items():
        mh = pkg.KmerMinHash(1000, 21, True, 42, 0, True, alphabet=alpha)
        mh.add_sequence(DNA96)
        assert (len(mh), int(mh.abunds_np().sum()), mh.mins[0]) == want, alpha


# ------------------------------------------------------------------------------------------------------------------
# 1. tile and run edges

@pytest.mark.parametrize("w", [7, 9, 10, 16, 42])
def test_tile_and_run_edges(pkg, geom, field, w):
    T, R = geom
    alpha = ALPHA_OF_W[w]
    n = 3 * T
    h = field_hashes(field, alpha, w)
    keep_alive, ptr = on_device(field)
    floor = 200 if alpha == "hp" else 6000          # hp: 2^42 words, but the field is checked window by window anyway
    check_field(pkg, alpha, w, ptr, n, [0, n], h, floor)                       # one record covering three tiles
    check_field(pkg, alpha, w, ptr, n, [0, T, 2 * T, n], h, floor)             # records ending exactly at the tile ends
    for cut in range(T - w - 1, T + w + 2):                                    # a boundary around the tile edge
        check_field(pkg, alpha, w, ptr, n, [0, cut, n], h, floor)
    for lane in (0, 1, 63, 64, T // R - 1):                                    # ... at each offset of these lanes' runs
        for k in range(R + w + 1):
            check_field(pkg, alpha, w, ptr, n, [0, T + lane * R + k, n], h, floor)
    for n_short in (2 * T + 1, 2 * T + 5, 2 * T + R - 1, 2 * T + R):           # the input ends inside the last tile's first run
        check_field(pkg, alpha, w, ptr, n_short, [0, n_short], h, floor // 2)
        check_field(pkg, alpha, w, ptr, n_short, [0, 2 * T - 3, n_short], h, floor // 2)
    del keep_alive


# ------------------------------------------------------------------------------------------------------------------
# 2. short records

@pytest.mark.parametrize("w", [9, 16, 42])
def test_short_records_in_every_order(pkg, geom, w):
    """records of 0, 1, W - 1, W, W + 1 bytes in all 120 orders behind a long record, so that they straddle the first
    tile's end; the last record of the batch has W - 1 bytes"""
    T, _ = geom
    alpha = ALPHA_OF_W[w]
    rng = np.random.default_rng(w)
    per = 3 * w + 1
    lead = max(200, T - 60 * per)                       # the 600 short records lie across the first tile's end (W = 42: across three)
    lens = [lead]
    for perm in itertools.permutations((0, 1, w - 1, w, w + 1)):
        lens += perm
    lens += [w - 1]
    data = rng.choice(LETTERS, size=sum(lens)).tobytes()
    off = np.concatenate(([0], np.cumsum(lens))).astype(np.uint64)
    recs = [data[int(a):int(b)] for a, b in zip(off, off[1:])]
    want = ar.amino_sketch(recs, alpha, 3 * w, 0, MAXH)
    assert len(want.mins) >= (200 if alpha == "hp" else 1000)
    mh = new_sketch(pkg, alpha, w)
    c = ar.counters(pkg, lambda: mh.add_proteins(recs))
    ar.same_state(mh, want)
    assert_route(c, w, 1)


@pytest.mark.parametrize("w", [1, 9])
def test_more_record_starts_than_threads(pkg, geom, field, w):
    """the whole first tile cut into 1-byte records (T starts for 256 threads), the second into 2-byte ones, then twenty
    zero-length records at one position inside the third, and a last record of W - 1"""
    T, _ = geom
    alpha = "dayhoff"
    n = 3 * T
    h = field_hashes(field, alpha, w)
    keep_alive, ptr = on_device(field)
    off = list(range(0, T)) + list(range(T, 2 * T, 2)) + [2 * T] + [2 * T + 1000] * 21 + [n - (w - 1), n]
    floor = 6 if w == 1 else 3000
    check_field(pkg, alpha, w, ptr, n, off, h, floor)
    # the zero-length records alone, at a tile end and inside a lane's run
    check_field(pkg, alpha, w, ptr, n, [0] + [T] * 21 + [T + 7] * 21 + [n], h, floor)
    check_field(pkg, alpha, w, ptr, n, [0] * 21 + [n] * 3, h, floor)
    del keep_alive


# ------------------------------------------------------------------------------------------------------------------
# 3. bytes

@pytest.mark.parametrize("alpha", ar.ALPHABETS)
def test_all_byte_values(pkg, alpha):
    rec = bytes(range(256)) * 2
    want = ar.amino_sketch([rec, rec[::-1]], alpha, 27, 0, MAXH)
    assert len(want.mins) >= {"protein": 400, "dayhoff": 60, "hp": 40}[alpha]
    mh = new_sketch(pkg, alpha, 9)
    c = ar.counters(pkg, lambda: mh.add_proteins([rec, rec[::-1]]))
    ar.same_state(mh, want)
    assert_route(c, 9, 1)
    if alpha == "protein":      # NUL, 0xFF and lower case are residues: the windows that hold them are there
        from pyoracle import hash_murmur
        for win in (bytes(range(0, 9)), bytes(range(247, 256)), bytes(range(0x60, 0x69)).upper(), b"\xff\xfe\xfd\xfc\xfb\xfa\xf9\xf8\xf7"):
            assert hash_murmur(win, 42) in set(mh.mins)


# ------------------------------------------------------------------------------------------------------------------
# 4. window lengths

@pytest.mark.parametrize("w", [1, 7, 8, 9, 10, 15, 16, 17, 32, 33, 42, 63, 64, 65, 100])
def test_window_lengths(pkg, geom, field, w):
    """murmur's block / tail edges (15, 16, 17; 32, 33; 63, 64) and the edge between the tiled and the byte-wise kernel
    (64, 65), over records of mixed lengths across three tiles"""
    T, R = geom
    alpha = ("protein", "dayhoff", "hp")[w % 3] if w > 1 else "protein"
    n = 3 * T
    h = field_hashes(field, alpha, w)
    keep_alive, ptr = on_device(field)
    off = [0, 5, 5 + w, 700, T - 1, T + R + 3, T + R + 3 + 2 * w, 2 * T + 40, n - w, n]
    floor = 15 if w == 1 else (200 if alpha == "hp" and w < 12 else 3000)
    check_field(pkg, alpha, w, ptr, n, off, h, floor)
    check_field(pkg, alpha, w, ptr, n, [0, n], h, floor)
    del keep_alive


# ------------------------------------------------------------------------------------------------------------------
# 5. pointer alignment

@pytest.mark.parametrize("misalign", [1, 3, 8, 15])
def test_unaligned_base_pointer(pkg, geom, field, misalign):
    T, R = geom
    n = 3 * T - 7
    keep_alive, ptr = on_device(field, misalign)
    for w in (9, 16, 42, 100):
        alpha = ALPHA_OF_W.get(w, "dayhoff")
        h = field_hashes(field, alpha, w)
        check_field(pkg, alpha, w, ptr, n, [0, T - 3, T + 2 * R + 1, 2 * T, n], h, 200 if alpha == "hp" else 3000)
    del keep_alive


# ------------------------------------------------------------------------------------------------------------------
# 6. sketch modes

def test_bottom_num_with_abundance_is_order_dependent(pkg):
    """num = 50 with abundances over 5 200 hp windows of 7: the last kept hash counts only the occurrences up to the point
    the sketch reached its final content (quirks Q3 / Q4), so the records in reverse order give other abundances -- in the
    restatement too, or the input would prove nothing"""
    rng = np.random.default_rng(6)
    data = rng.choice(LETTERS, size=5200).tobytes()
    cuts = [0, 300, 1100, 1800, 2600, 3700, 4400, 5200]
    recs = [data[a:b] for a, b in zip(cuts, cuts[1:])]
    fwd, rev = ar.amino_sketch(recs, "hp", 21, 50, 0), ar.amino_sketch(recs[::-1], "hp", 21, 50, 0)
    assert len(fwd.mins) == 50 and fwd.abunds != rev.abunds
    for order, want in ((recs, fwd), (recs[::-1], rev)):
        mh = new_sketch(pkg, "hp", 7, num=50, max_hash=0)
        c = ar.counters(pkg, lambda: mh.add_proteins(order))
        ar.same_state(mh, want)
        assert_route(c, 7)
    # the same through single calls, queued work in between: call order is stream order
    mh = new_sketch(pkg, "hp", 7, num=50, max_hash=0)
    want = ar.new_sketch(21, 50, 0)
    for i, r in enumerate(recs):
        mh.add_protein(r)
        ar.amino_sketch([r], "hp", 21, into=want)
        mh.add_word(b"hphphph"[: 7 - (i & 1)])
        want.add_word(b"hphphph"[: 7 - (i & 1)])
        mh.add_hash(1000 + i)
        want.add_hash(1000 + i)
    ar.same_state(mh, want)


def test_growing_chunk_loop(pkg):
    """num = 1000 over 72 000 windows with 600 distinct ones: the one-pass attempt keeps fewer than num distinct hashes and
    applies nothing; the growing-chunk loop then launches over [0, 65 536) and [65 536, 72 000) -- range_lo != 0"""
    rng = np.random.default_rng(7)
    data = rng.choice(LETTERS, size=600).tobytes() * 120
    want = ar.amino_sketch([data], "protein", 27, 1000, 0)
    assert len(want.mins) == 600 and sum(want.abunds) == len(data) - 8
    mh = new_sketch(pkg, "protein", 9, num=1000, max_hash=0)
    c = ar.counters(pkg, lambda: mh.add_protein(data))
    ar.same_state(mh, want)
    assert_route(c, 9, 3)


def test_order_dependent_mode_beyond_one_chunk(pkg):
    """num and max_hash both set: the windows are replayed through add_hash in stream order, in chunks of 2^24 positions.
    One batch of 2^24 + 6000 bytes whose content is three records -- at the start, across position 2^24, at the end --
    between filler records of W - 1 bytes, which add nothing: the restatement sees the three records alone (hashing 16
    million windows in Python is out of reach of a quick test; the launch still walks all the bytes and two chunks)."""
    w, alpha = 9, "hp"
    n = (1 << 24) + 6000
    rng = np.random.default_rng(8)
    data = rng.choice(LETTERS, size=n)
    isl = [(0, 3000), ((1 << 24) - 1000, (1 << 24) + 1000), (n - 1500, n)]
    parts = [np.array([0], dtype=np.uint64)]
    for (a0, a1), (b0, _) in zip(isl, isl[1:]):
        parts.append(np.arange(a1, b0, w - 1, dtype=np.uint64))
        parts.append(np.array([b0], dtype=np.uint64))
    parts.append(np.array([n], dtype=np.uint64))
    off = np.unique(np.concatenate(parts))
    assert (np.diff(off.astype(np.int64)) > 0).all() and sorted(np.diff(off.astype(np.int64)))[-4] <= w - 1
    recs = [data[a:b].tobytes() for a, b in isl]
    case = dict(num=50, max_hash=1 << 63)
    want = ar.amino_sketch(recs, alpha, 3 * w, 50, 1 << 63)
    assert len(want.mins) >= 200 and want.abunds != ar.amino_sketch(recs[::-1], alpha, 3 * w, 50, 1 << 63).abunds
    keep_alive, ptr = on_device(data.tobytes())
    mh = new_sketch(pkg, alpha, w, **case)
    c = ar.counters(pkg, lambda: mh.add_proteins_dev(ptr, n, off))
    ar.same_state(mh, want)
    assert_route(c, w, 2)
    del keep_alive


def test_scaled_sketch_across_calls(pkg, geom, field):
    """two calls into one scaled sketch (resident in HBM in between) == one call == merge of the halves"""
    T, _ = geom
    thr = (1 << 64) // 4
    a, b = field[:T + 333], field[T + 333:]
    want = ar.amino_sketch([a, b], "dayhoff", 27, 0, thr)
    assert len(want.mins) >= 1500
    one, two, ha, hb = (new_sketch(pkg, "dayhoff", 9, max_hash=thr) for _ in range(4))
    one.add_proteins([a, b])
    c = ar.counters(pkg, lambda: (two.add_protein(a), two.add_protein(b)), names=("amino_tiled", "sketch_to_host"))
    assert c == {"amino_tiled": 2, "sketch_to_host": 0}
    ha.add_protein(a); hb.add_protein(b); ha.merge(hb)
    for mh in (one, two, ha):
        ar.same_state(mh, want)


def test_candidate_overflow_is_rerun(pkg):
    """a record of one letter, 10^6 long, with max_hash = the hash of its only window: every window passes where the
    uniform estimate expects a fraction, the candidate buffer overflows and the chunk is run again with the exact size.
    The letter is the one whose hash is the largest below 0.7 * 2^64 (the estimate has 25 % head-room).  Closed form:
    one hash, n - W + 1 times; one below it, nothing."""
    from pyoracle import hash_murmur
    n, w = 1_000_000, 9
    hs = {chr(c): hash_murmur(bytes([c]) * w, 42) for c in LETTERS}
    letter, hv = max(((k, v) for k, v in hs.items() if v < 0.7 * 2 ** 64), key=lambda kv: kv[1])
    assert hv > 0.05 * 2 ** 64
    rec = letter.encode() * n
    mh = new_sketch(pkg, "protein", w, max_hash=hv)
    c = ar.counters(pkg, lambda: mh.add_protein(rec))
    assert mh.mins == [hv] and mh.abunds == [n - w + 1]
    assert c["chunk_rerun"] >= 1 and c["amino_tiled"] >= 2, c
    mh = new_sketch(pkg, "protein", w, max_hash=hv - 1)
    mh.add_protein(rec)
    assert mh.mins == [] and mh.abunds == []


# ------------------------------------------------------------------------------------------------------------------
# 7. translated input in the reduced alphabets

def rand_dna_records(seed, lens):
    rng = random.Random(seed)
    out = []
    for n in lens:
        s = bytearray(rng.choice(b"ACGTacgt") for _ in range(n))
        for i in range(n):
            if rng.random() < 0.01:
                s[i] = ord("N")
        out.append(bytes(s))
    return out


@pytest.mark.parametrize("alpha", ["dayhoff", "hp"])
@pytest.mark.parametrize("ksize", [21, 27, 30, 48])
def test_translated_input(pkg, alpha, ksize):
    """add_sequences_dev on a dayhoff / hp sketch: the protein arm with every residue mapped.  ksize 21 / 27 / 30 take the
    one-pass kernel (N bytes make spliced spans for its second launch), 48 the two-pass path; a record of b"\\xc3\\xa9"
    forces the two-pass path at every ksize"""
    recs = rand_dna_records(ksize, [0, 20, ksize - 1, ksize, 150, 999, 1200, ksize + 1])
    clean = bytes(random.Random(1).choice(b"ACGT") for _ in range(300))
    recs.append(clean[:150] + b"N" + clean[150:])                      # one spliced span in an otherwise clean record
    fused = ksize // 3 in (7, 9, 10)
    for extra in ([], [b"\xc3\xa9"]):
        rr = recs + extra
        want = ar.translated_sketch(rr, alpha, ksize, 0, MAXH)
        assert len(want.mins) >= (100 if alpha == "hp" and ksize < 40 else 2000)
        data = b"".join(rr)
        off = np.concatenate(([0], np.cumsum([len(r) for r in rr]))).astype(np.uint64)
        keep_alive, ptr = on_device(data)
        mh = new_sketch(pkg, alpha, ksize // 3)
        assert mh.ksize == ksize
        c = ar.counters(pkg, lambda: mh.add_sequences_dev(ptr, len(data), off, True))
        ar.same_state(mh, want)
        assert c["amino_tiled"] == 0 and c["amino_generic"] == 0, c
        if fused and not extra:
            assert c["protein_fused"] >= 1 and c["translate"] == 0 and c["hash_windows"] == 0, c
        else:
            assert c["translate"] == 1 and c["hash_windows"] >= 1 and (c["protein_fused"] >= 1) == fused, c
        del keep_alive
    # one record at a time through add_sequence (queued, then one batch): the same sketch
    mh = new_sketch(pkg, alpha, ksize // 3)
    for r in recs:
        mh.add_sequence(r)
    ar.same_state(mh, ar.translated_sketch(recs, alpha, ksize, 0, MAXH))


# ------------------------------------------------------------------------------------------------------------------
# 8. downstream of a sketch

def test_downstream_of_dayhoff_sketches(pkg):
    """a resident index of dayhoff sketches built from amino-acid input answers find, gather and compare exactly like an
    index of sketches filled with the restatement's hashes through add_many; a protein query is refused with 102"""
    from importlib import import_module
    index = import_module(pkg.__name__ + ".index")
    rng = np.random.default_rng(9)
    thr = (1 << 64) // 8
    base = [rng.choice(LETTERS, size=3000).tobytes() for _ in range(4)]
    genomes = [[base[0], base[1]], [base[1], base[2]], [base[2]], [base[3], base[0][:1500]]]
    query_recs = [base[0][:2000], base[2][500:2500], base[3][100:900]]
    built, ref = [], []
    for recs in genomes + [query_recs]:
        g = new_sketch(pkg, "dayhoff", 9, max_hash=thr)
        g.add_proteins(recs)
        want = ar.amino_sketch(recs, "dayhoff", 27, 0, thr)
        ar.same_state(g, want)
        r = new_sketch(pkg, "dayhoff", 9, max_hash=thr)
        r.add_many_with_abund(list(zip(want.mins, want.abunds)))
        ar.same_state(r, want)
        built.append(g); ref.append(r)
    qa, qb = built.pop(), ref.pop()
    assert len(qa) >= 300
    ia, ib = index.ResidentIndex(built), index.ResidentIndex(ref)
    for containment in (False, True):
        fa = ia.find(qa, 0.05, containment)
        assert fa == ib.find(qb, 0.05, containment) and len(fa) >= 2
    ga, gb = ia.gather(qa), ib.gather(qb)
    assert len(ga.rows) >= 3 and ga.rows == gb.rows and (ga.assigned == gb.assigned).all()
    ca, cb = ia.compare(ia, want=("jaccard", "common", "containment")), ib.compare(ib, want=("jaccard", "common", "containment"))
    for k in ca:
        assert (ca[k] == cb[k]).all()
    assert (ca["common"] > 0).sum() >= 8
    prot = new_sketch(pkg, "protein", 9, max_hash=thr)
    prot.add_proteins(query_recs)
    for fn in (lambda: ia.find(prot, 0.05), lambda: ia.gather(prot), lambda: prot.compare(qa),
               lambda: index.ResidentIndex(built + [prot]).compare(ia)):
        with pytest.raises(pkg.SourmashError) as e:
            fn()
        assert e.value.code == 102


def test_records_from_a_protein_fasta(pkg):
    """smh_add_records_protein on a parsed protein FASTA (wrapped lines, CRLF, a lower-case record, an empty record) equals
    smh_add_proteins on the same records cut by hand"""
    from importlib import import_module
    fastx = import_module(pkg.__name__ + ".fastx")
    rng = np.random.default_rng(10)
    recs = [rng.choice(LETTERS, size=n).tobytes() for n in (700, 61, 0, 8, 5000, 9)]
    recs[1] = recs[1].lower()
    text = b""
    for i, r in enumerate(recs):
        eol = b"\r\n" if i == 4 else b"\n"
        text += b">p%d some protein" % i + eol
        text += b"".join(r[j:j + 60] + eol for j in range(0, len(r), 60))
    for alpha in ("dayhoff", "protein"):
        want = ar.amino_sketch(recs, alpha, 27, 0, MAXH)
        assert len(want.mins) >= 4000
        parsed = fastx.Records.parse(text, "fasta")
        assert len(parsed) == len(recs)
        a, b = new_sketch(pkg, alpha, 9), new_sketch(pkg, alpha, 9)
        c = ar.counters(pkg, lambda: a.add_records_protein(parsed))
        b.add_proteins(recs)
        ar.same_state(a, want)
        ar.same_state(b, want)
        assert_route(c, 9, 1)
