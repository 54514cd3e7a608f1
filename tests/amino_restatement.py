"""The alphabets and the amino-acid input of include/sourmash_amd.h ("Alphabets and amino-acid input"), restated in plain
Python on the oracle's primitives (MinHash.add_word, to_aa, revcomp).  No product import; tests/test_amino_rules.py checks
this file against the rules as written and against the oracle, the GPU tests compare the library with it bit for bit.

    amino_sketch(records, alphabet, ksize, ...)       every window of ksize // 3 bytes of every record, in order
    translated_sketch(records, alphabet, ksize, ...)  add_sequence's protein arm with every residue mapped before hashing"""
import pyoracle

ALPHABETS = ("protein", "dayhoff", "hp")

DAYHOFF = {"a": "C", "b": "AGPST", "c": "DENQ", "d": "HKR", "e": "ILMV", "f": "FWY"}
HP = {"h": "AFGILMPVWY", "p": "NCSTDERHKQ"}
LETTERS = "ACDEFGHIKLMNPQRSTVWY"          # the 20 amino acids

_UPPER = bytes.maketrans(bytes(range(ord("a"), ord("z") + 1)), bytes(range(ord("A"), ord("Z") + 1)))


def _table(groups):
    """upper-cased byte -> class letter; '*' is itself, every other byte is X"""
    t = bytearray(b"X" * 256)
    t[ord("*")] = ord("*")
    for cls, members in groups.items():
        for m in members:
            t[ord(m)] = ord(cls)
    return bytes(t)


TABLES = {"protein": bytes(range(256)), "dayhoff": _table(DAYHOFF), "hp": _table(HP)}


def encode(seq, alphabet):
    """what a record's bytes are hashed as: upper-cased (a-z only), then mapped"""
    return bytes(seq).translate(_UPPER).translate(TABLES[alphabet])


def new_sketch(ksize, num=0, max_hash=0, track=True, seed=42):
    return pyoracle.MinHash(num, ksize, True, seed, max_hash, track)


def amino_sketch(records, alphabet, ksize, num=0, max_hash=0, track=True, seed=42, into=None):
    mh = into if into is not None else new_sketch(ksize, num, max_hash, track, seed)
    w = ksize // 3
    if w == 0:
        raise pyoracle.OraclePanic("windows(0)")
    for rec in records:
        e = encode(rec, alphabet)
        for i in range(len(e) - w + 1):
            mh.add_word(e[i:i + w])
    return mh


def translated_sketch(records, alphabet, ksize, num=0, max_hash=0, track=True, seed=42, into=None):
    """reference src/lib.rs:275-302 with map() between to_aa and windows(); records shorter than ksize add nothing"""
    mh = into if into is not None else new_sketch(ksize, num, max_hash, track, seed)
    w = ksize // 3
    for rec in records:
        s = bytes(rec).translate(_UPPER)
        if len(s) < ksize:
            continue
        rc = pyoracle.revcomp(s)
        for frame in range(3):
            for strand in (s, rc):
                aa = pyoracle.to_aa(strand[frame:])
                if w == 0:
                    raise pyoracle.OraclePanic("windows(0)")
                e = aa.translate(TABLES[alphabet])
                for i in range(len(e) - w + 1):
                    mh.add_word(e[i:i + w])
    return mh


def window_hashes(data, alphabet, w, seed=42):
    """murmur64 (what add_word hashes) of the window at every start of `data` read as ONE record, in order"""
    e = encode(data, alphabet)
    return [pyoracle.hash_murmur(e[i:i + w], seed) for i in range(len(e) - w + 1)]


def starts_inside_records(n, offsets, w):
    """the window starts i of a batch of n bytes cut at `offsets` (ascending, repeats = empty records, first 0, last n)
    whose w bytes lie inside one record: no record start in (i, i + w - 1] and i + w <= n -- ascending, a numpy array"""
    import numpy as np
    if n < w:
        return np.zeros(0, dtype=np.int64)
    mark = np.zeros(n + w + 1, dtype=np.int64)
    cuts = np.unique(np.asarray(offsets, dtype=np.int64))
    mark[cuts[(cuts > 0) & (cuts < n)]] = 1
    upto = np.cumsum(mark)                          # record starts at positions <= x
    i = np.arange(n - w + 1)
    return i[upto[i + w - 1] - upto[i] == 0]


def full_state(hashes):
    """(mins, abunds) of a tracked sketch that keeps everything (scaled with max_hash = 2^64 - 1, or bottom-num with num
    above the distinct count) after add_hash of every hash: ascending distinct hashes and how often each came (numpy)"""
    import numpy as np
    mins, abunds = np.unique(np.asarray(hashes, dtype=np.uint64), return_counts=True)
    return mins, abunds.astype(np.uint64)


def window_count(lengths, ksize):
    w = ksize // 3
    return sum(max(0, n - w + 1) for n in lengths)


def same_state(g, o):
    """a library sketch and an oracle sketch hold the same hashes and abundances"""
    import numpy as np
    gm, om = g.mins_np(), np.asarray(o.mins, dtype=np.uint64)
    assert gm.shape == om.shape and (gm == om).all()
    if o.abunds is not None:
        ga, oa = g.abunds_np(), np.asarray(o.abunds, dtype=np.uint64)
        assert ga.shape == oa.shape and (ga == oa).all()


def counters(pkg, fn, names=("amino_tiled", "amino_generic", "protein_fused", "translate", "hash_windows", "chunk_rerun")):
    """launches of the named kernels / events while `fn` runs (smh_profile_get)"""
    import ctypes as C
    L = pkg.lib()
    L.smh_profile_reset(); L.smh_profile_enable(1)
    try:
        fn()
    finally:
        L.smh_profile_enable(0)
    out = {}
    for name in names:
        ms, n = C.c_double(), C.c_uint64()
        L.smh_profile_get(name.encode(), C.byref(ms), C.byref(n))
        out[name] = n.value
    return out
