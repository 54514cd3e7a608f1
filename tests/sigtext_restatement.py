"""The rules of signature JSON written on the device (include/sourmash_amd.h, "Signature JSON written on the device";
DESIGN.md 3.28), restated in plain Python: str(), hashlib.md5 and nothing from the code under test.  This file is normative:
the host build of csrc/sigtext_core.hpp and the kernels are compared against it, and it is compared against the host writer
(signatures_save_buffer) and against the md5sum strings sourmash itself wrote into the fixtures.

A sketch is a dict: num, ksize, seed, max_hash, mins (ascending ints), abunds (None or one int per hash), molecule (a string of
MOLECULES)."""
import glob
import hashlib
import json
import os
import random

MOLECULES = ("DNA", "protein", "dayhoff", "hp")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# the digit-count edges: 0, 9, 10, 99, 100, ... every 10^d - 1 and 10^d up to 10^19, 2^32 - 1, 2^32, 2^64 - 1
EDGE_HASHES = sorted({0, 2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1} | {10 ** d for d in range(20)} | {10 ** d - 1 for d in range(1, 20)})
EDGE_ABUNDS = sorted({1, 2 ** 32 - 1} | {10 ** d for d in range(10)} | {10 ** d - 1 for d in range(1, 10)})
NAMES = ['quote " inside', "back\\slash", "ctl \x01 byte", "a\ttab", "café 中文 \U0001f9ec", "", None]
PAD_LENGTHS = (1, 2, 55, 56, 57, 63, 64, 65, 119, 120, 121, 128)   # md5 message lengths around RFC 1321's padding


def json_string(s):
    """a name or filename as serde_json writes it; None is null"""
    if s is None:
        return "null"
    short = {'"': '\\"', "\\": "\\\\", "\b": "\\b", "\f": "\\f", "\n": "\\n", "\r": "\\r", "\t": "\\t"}
    return '"' + "".join(short.get(c) or ("\\u%04x" % ord(c) if ord(c) < 0x20 else c) for c in s) + '"'


def md5_hex(ksize, mins):
    return hashlib.md5((str(ksize) + "".join(str(h) for h in mins)).encode()).hexdigest()


def signature_text(sk, name, filename):
    out = ('{"class":"sourmash_signature","email":"","hash_function":"0.murmur64","filename":%s,"name":%s,"license":"CC0","signatures":['
           % (json_string(filename), json_string(name)))
    out += '{"num":%d,"ksize":%d,"seed":%d,"max_hash":%d,"mins":[%s],"md5sum":"%s"' % (
        sk["num"], sk["ksize"], sk["seed"], sk["max_hash"], ",".join(str(h) for h in sk["mins"]), md5_hex(sk["ksize"], sk["mins"]))
    if sk["abunds"] is not None:
        out += ',"abundances":[%s]' % ",".join(str(a) for a in sk["abunds"])
    return out + ',"molecule":"%s"}],"version":0.4}' % sk["molecule"]


def text(sketches, names=None, filenames=None, doc_starts=None):
    """(the whole text as bytes, doc_offsets): document d holds sketches[doc_starts[d]:doc_starts[d + 1]]"""
    n = len(sketches)
    names = [None] * n if names is None else names
    filenames = [None] * n if filenames is None else filenames
    doc_starts = [0, n] if doc_starts is None else list(doc_starts)
    out, offs = b"", [0]
    for a, b in zip(doc_starts, doc_starts[1:]):
        out += ("[" + ",".join(signature_text(sketches[v], names[v], filenames[v]) for v in range(a, b)) + "]").encode("utf-8")
        offs.append(len(out))
    return out, offs


def text_len(sketches, names=None, filenames=None, doc_starts=None):
    """len(text(...)[0]) by arithmetic on one representative of equal sketches (the text past 4 GiB is never built on the host)"""
    n = len(sketches)
    names = [None] * n if names is None else names
    filenames = [None] * n if filenames is None else filenames
    doc_starts = [0, n] if doc_starts is None else list(doc_starts)
    seen, total = {}, 0
    for a, b in zip(doc_starts, doc_starts[1:]):
        total += 2 + max(b - a - 1, 0)
        for v in range(a, b):
            key = (id(sketches[v]), names[v], filenames[v])
            if key not in seen:
                seen[key] = len(signature_text(sketches[v], names[v], filenames[v]).encode("utf-8"))
            total += seen[key]
    return total


def sketch(mins, abunds=None, num=0, ksize=21, seed=42, max_hash=2 ** 64 - 1, molecule="DNA"):
    return {"num": num, "ksize": ksize, "seed": seed, "max_hash": max_hash, "mins": list(mins), "abunds": None if abunds is None else list(abunds),
            "molecule": molecule}


def hashes_for_length(length, ksize):
    """ascending hashes for which the md5 message -- str(ksize) and their digits -- is `length` bytes long; None if ksize alone
    is longer"""
    r = length - len(str(ksize))
    if r < 0:
        return None
    ones = r if r <= 10 else (10 if (r - 10) % 2 == 0 else 9)
    twos = (r - ones) // 2
    assert twos <= 90 and ones + 2 * twos == r
    return list(range(ones)) + list(range(10, 10 + twos))


def fixture_paths():
    return [os.path.join(GOLDEN, "genome-s10+s11.sig")] + sorted(glob.glob(os.path.join(GOLDEN, "sbt_v5", "*.sig")))


def fixture_sketches():
    """[(sketch, name, filename, md5sum as sourmash wrote it)] of every sketch of the fixtures, in file order"""
    out = []
    for path in fixture_paths():
        with open(path) as fh:
            for sig in json.load(fh):
                for sk in sig["signatures"]:
                    # (the loader reads `molecule` in any case; the writer's spelling is MOLECULES')
                    molecule = {m.lower(): m for m in MOLECULES}[sk.get("molecule", "DNA").lower()]
                    out.append((sketch(sk["mins"], sk.get("abundances"), sk["num"], sk["ksize"], sk["seed"], sk["max_hash"], molecule),
                                sig.get("name"), sig.get("filename"), sk["md5sum"]))
    return out


def crafted_groups():
    """[(label, sketches, names, filenames)]: every group's sketches agree on whether they carry abundances, as the nodes of
    one index do"""
    edge_abunds = (EDGE_ABUNDS * 3)[:len(EDGE_HASHES)]
    groups = []
    plain = [sketch(EDGE_HASHES), sketch([], ksize=31), sketch([7], num=500, max_hash=0, ksize=7),
             sketch(EDGE_HASHES[:5], molecule="protein", ksize=30), sketch(EDGE_HASHES[3:9], molecule="dayhoff", ksize=33),
             sketch(EDGE_HASHES[-4:], molecule="hp", ksize=100, seed=7), sketch(range(1, 300, 7), num=1000, max_hash=0)]
    groups.append(("plain", plain, NAMES, list(reversed(NAMES))))
    abund = [sketch(EDGE_HASHES, edge_abunds), sketch([], []), sketch([5, 6], [2 ** 32 - 1, 1], num=20, max_hash=0),
             sketch(EDGE_HASHES[:7], EDGE_ABUNDS[:7], molecule="protein"), sketch([10 ** 19], [10 ** 9], molecule="hp"),
             sketch(EDGE_HASHES[2:4], [9, 10], molecule="dayhoff"), sketch([2 ** 64 - 1], [4294967295])]
    groups.append(("abund", abund, list(reversed(NAMES)), NAMES))
    groups.append(("nulls", plain[:3], None, None))
    for k in (7, 21, 100):
        pads = [sketch(h, ksize=k) for h in (hashes_for_length(L, k) for L in PAD_LENGTHS) if h is not None]
        groups.append(("pad_k%d" % k, pads, None, None))
    return groups


def random_index(rng):
    """0-6 nodes of 0-300 values: (sketches, names, filenames, doc_starts)"""
    n = rng.randrange(7)
    with_abunds = rng.random() < 0.5
    sketches = []
    for _ in range(n):
        m = rng.randrange(301)
        mins = sorted({rng.randrange(10 ** rng.randrange(1, 21)) % 2 ** 64 for _ in range(m)})
        abunds = [rng.randrange(10 ** rng.randrange(1, 11)) % 2 ** 32 for _ in mins] if with_abunds else None
        scaled = rng.random() < 0.5
        sketches.append(sketch(mins, abunds, 0 if scaled else rng.randrange(1, 2000), rng.choice((7, 21, 31, 100)), rng.randrange(100),
                               2 ** 64 - 1 if scaled else 0, rng.choice(MOLECULES)))
    names = [rng.choice(NAMES) for _ in range(n)] if rng.random() < 0.7 else None
    filenames = [rng.choice(NAMES) for _ in range(n)] if rng.random() < 0.7 else None
    doc_starts = None
    if rng.random() < 0.6:
        doc_starts = [0] + sorted(rng.randrange(n + 1) for _ in range(rng.randrange(4))) + [n]
    return sketches, names, filenames, doc_starts


def random_indexes(count, seed=20251):
    rng = random.Random(seed)
    return [random_index(rng) for _ in range(count)]
