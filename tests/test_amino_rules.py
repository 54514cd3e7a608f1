"""The alphabets and the amino-acid input rules (include/sourmash_amd.h), without a device: the restatement
tests/amino_restatement.py against the rules as written, against the oracle and against the known answers; and what the
library does with a molecule on the host -- constructor, compatibility, signature JSON, the refusals."""
import ctypes as C
import itertools
import json
import random

import pytest

import amino_restatement as ar

U64P = C.POINTER(C.c_uint64)
REC50 = b"MVLSPADKTNVKAAWGKVGAHAGEYGAEALERMFLSFPTTKTYFPHF*xb"
DNA96 = b"ATGGTGCTGTCTCCTGCCGACAAGACCAACGTCAAGGCCGCCTGGGGTAAGGTCGGCGCGCACGCTGGCGAGTATGGTGCGGAGGCCCTGGAGAGG"
# (distinct hashes, sum of abundances, smallest hash) into num=1000, max_hash=0, abundances tracked, seed 42
KNOWN = {
    ("protein", 21): (44, 44, 88833800559946942), ("protein", 27): (42, 42, 1160878527000605285),
    ("protein", 48): (35, 35, 1209005312177089901),
    ("dayhoff", 21): (44, 44, 109835400199548061), ("dayhoff", 27): (42, 42, 1192610630844060659),
    ("dayhoff", 48): (35, 35, 112565541511913274),
    ("hp", 21): (31, 44, 208447871966926936), ("hp", 27): (36, 42, 662985850476107860), ("hp", 48): (35, 35, 6705633307785086),
}
KNOWN_TRANSLATED = {"dayhoff": (151, 152, 29833093626199857), "hp": (87, 152, 208447871966926936)}
MOLS = ("DNA", "protein", "dayhoff", "hp")


def test_tables_partition_the_letters():
    for groups, n in ((ar.DAYHOFF, 6), (ar.HP, 2)):
        members = "".join(groups.values())
        assert len(groups) == n and sorted(members) == sorted(ar.LETTERS)       # every letter in exactly one class
    assert ar.DAYHOFF == {"a": "C", "b": "AGPST", "c": "DENQ", "d": "HKR", "e": "ILMV", "f": "FWY"}
    assert {k: sorted(v) for k, v in ar.HP.items()} == {"h": sorted("AFGILMPVWY"), "p": sorted("NCSTDERHKQ")}


def test_all_256_bytes_map_as_the_rules_say():
    for b in range(256):
        u = b - 32 if ord("a") <= b <= ord("z") else b
        assert ar.encode(bytes([b]), "protein") == bytes([u])
        for name, groups in (("dayhoff", ar.DAYHOFF), ("hp", ar.HP)):
            want = "X"
            if u == ord("*"):
                want = "*"
            for cls, members in groups.items():
                if chr(u) in members:
                    want = cls
            assert ar.encode(bytes([b]), name) == want.encode(), (name, b)
    assert ar.encode(REC50, "dayhoff") == b"eeebbbcdbcedbbfbdebbdbbcfbbcbecdefebfbbbdbffbdf*XX"


def test_identity_translated_sketch_is_the_oracle(pyoracle):
    rng = random.Random(5)
    for ksize in (21, 27, 48):
        recs = []
        for n in (0, 20, 26, 95, 200, 333):
            s = bytearray(rng.choice(b"ACGTacgt") for _ in range(n))
            for i in range(n):
                if rng.random() < 0.03:
                    s[i] = ord("N")
            recs.append(bytes(s))
        o = pyoracle.MinHash(0, ksize, True, 42, (1 << 64) - 1, True)
        for r in recs:
            o.add_sequence(r)
        mine = ar.translated_sketch(recs, "protein", ksize, 0, (1 << 64) - 1)
        assert len(o.mins) > 300 and mine.mins == o.mins and mine.abunds == o.abunds


def test_known_answers(pyoracle):
    assert pyoracle.hash_murmur(b"bebbbbc", 42) == 17280634798361449420
    assert pyoracle.hash_murmur(b"hhhphhp", 42) == 15140769491848236245
    for (alpha, ksize), (distinct, total, smallest) in KNOWN.items():
        mh = ar.amino_sketch([REC50], alpha, ksize, 1000, 0)
        assert (len(mh.mins), sum(mh.abunds), mh.mins[0]) == (distinct, total, smallest), (alpha, ksize)
    for alpha, (distinct, total, smallest) in KNOWN_TRANSLATED.items():
        mh = ar.translated_sketch([DNA96], alpha, 21, 1000, 0)
        assert (len(mh.mins), sum(mh.abunds), mh.mins[0]) == (distinct, total, smallest), alpha
    o = pyoracle.MinHash(1000, 21, True, 42, 0, True)
    o.add_sequence(DNA96)
    mh = ar.translated_sketch([DNA96], "protein", 21, 1000, 0)
    assert mh.mins == o.mins and mh.abunds == o.abunds


def test_fast_restatement_is_the_add_word_one():
    """window_hashes + starts_inside_records + full_state (what the GPU sweeps use, one murmur per window of the field) give
    the state amino_sketch builds record by record with add_word -- empty, short and repeated records included"""
    rng = random.Random(11)
    data = bytes(rng.choice(b"ACDEFGHIKLMNPQRSTVWYacdxz*\x00\xff") for _ in range(400)) * 2
    n = len(data)
    for w, alpha in ((1, "hp"), (7, "dayhoff"), (9, "protein"), (16, "hp"), (42, "dayhoff")):
        offsets = [0, 0, 3, 3, 3, 50, 50 + w - 1, 50 + 2 * w - 1, 300, 301, 302, 420, 420, n - w + 1, n]
        recs = [data[a:b] for a, b in zip(offsets, offsets[1:])]
        want = ar.amino_sketch(recs, alpha, 3 * w, 0, (1 << 64) - 1)
        h = ar.window_hashes(data, alpha, w)
        keep = ar.starts_inside_records(n, offsets, w)
        assert len(keep) == ar.window_count([len(r) for r in recs], 3 * w) > 200
        mins, abunds = ar.full_state([h[i] for i in keep])
        assert mins.tolist() == want.mins and abunds.tolist() == want.abunds


# ---------------------------------------------------------------------------------------------- through the library, no device

def _sigmod(pkg):
    from importlib import import_module
    return import_module(pkg.__name__ + ".signature")


def _new(L, mol, ksize=27, num=0, max_hash=1 << 60, track=True):
    p = L.smh_kmerminhash_new_molecule(num, ksize, mol, 42, max_hash, track)
    assert p
    return p


def test_constructor_and_getters(pkg, pkg_lib):
    L = pkg_lib
    for mol in range(4):
        p = _new(L, mol)
        assert L.smh_kmerminhash_molecule(p) == mol
        assert L.kmerminhash_is_protein(p) == (mol != 0)
        L.kmerminhash_free(p)
    for prot in (False, True):
        p = L.kmerminhash_new(0, 27, prot, 42, 1 << 60, False)
        assert L.smh_kmerminhash_molecule(p) == (1 if prot else 0)
        L.kmerminhash_free(p)
    L.sourmash_err_clear()
    assert not L.smh_kmerminhash_new_molecule(0, 27, 4, 42, 1 << 60, False) and L.sourmash_err_get_last_code() == 3
    L.sourmash_err_clear()
    for alpha in ar.ALPHABETS:
        mh = pkg.KmerMinHash(0, 27, max_hash=1 << 60, alphabet=alpha)
        assert mh.molecule == alpha and mh.is_protein
    assert pkg.KmerMinHash(0, 27).molecule == "DNA" and pkg.KmerMinHash(0, 27, True).molecule == "protein"
    with pytest.raises(ValueError):
        pkg.KmerMinHash(0, 27, alphabet="DNA")


def test_differing_molecules_are_incompatible(pkg, pkg_lib):
    L = pkg_lib
    ps = [_new(L, mol) for mol in range(4)]
    for a, b in itertools.product(range(4), repeat=2):
        rc = L.smh_check_compatible(ps[a], ps[b])
        assert rc == (0 if a == b else 102), (a, b)
    L.sourmash_err_clear()
    # merge goes through the same check (add_from checks nothing, as in the reference); a copy carries the molecule
    d, h = pkg.KmerMinHash(0, 27, max_hash=1 << 60, alphabet="dayhoff"), pkg.KmerMinHash(0, 27, max_hash=1 << 60, alphabet="hp")
    with pytest.raises(pkg.SourmashError) as e:
        d.merge(h)
    assert e.value.code == 102
    sig = _sigmod(pkg).Signature()
    sig.push_mh(d)
    assert sig.first_mh().molecule == "dayhoff"
    for p in ps:
        L.kmerminhash_free(p)


def test_signature_json_round_trip(pkg):
    sigmod = _sigmod(pkg)
    sigs = []
    for i, alpha in enumerate(("dayhoff", "hp", "protein")):
        mh = pkg.KmerMinHash(0, 27, max_hash=1 << 62, track_abundance=True, alphabet=alpha)
        for h in (5 + i, 77, 1 << 40):
            mh.add_hash(h)
        s = _sigmod(pkg).Signature()
        s.name = alpha
        s.push_mh(mh)
        sigs.append(s)
    dna = pkg.KmerMinHash(0, 27, max_hash=1 << 62)
    dna.add_hash(9)
    s = _sigmod(pkg).Signature(); s.name = "DNA"; s.push_mh(dna)
    sigs.append(s)
    text = sigmod.save_signatures(sigs)
    assert [d["signatures"][0]["molecule"] for d in json.loads(text)] == ["dayhoff", "hp", "protein", "DNA"]
    back = sigmod.load_signatures_buffer(text.encode())
    assert [b.first_mh().molecule for b in back] == ["dayhoff", "hp", "protein", "DNA"]
    for a, b in zip(sigs, back):
        assert a == b and a.first_mh().mins == b.first_mh().mins
    assert not (sigs[0] == sigs[1])
    for mt, want in (("dayhoff", ["dayhoff"]), ("DAYHOFF", ["dayhoff"]), ("Hp", ["hp"]), ("protein", ["protein"]), ("dna", ["DNA"])):
        got = sigmod.load_signatures_buffer(text.encode(), moltype=mt)
        assert [g.first_mh().molecule for g in got] == want, mt
    # any other string still reads as DNA (quirk Q9)
    odd = json.loads(text)[:1]
    odd[0]["signatures"][0]["molecule"] = "Dayhoff"
    assert sigmod.load_signatures_buffer(json.dumps(odd).encode())[0].first_mh().molecule == "DNA"


def test_refusals_need_no_device(pkg_lib):
    L = pkg_lib
    off = (C.c_uint64 * 2)(0, len(REC50))
    dna = _new(L, 0)
    for rc in (L.smh_add_protein(dna, REC50, len(REC50)), L.smh_add_proteins(dna, REC50, off, 1),
               L.smh_add_proteins_dev(dna, None, 0, off, 0, None)):
        assert rc == 3                                        # SOURMASH_ERROR_CODE_MSG, before the device is touched
    assert L.kmerminhash_get_mins_size(dna) == 0
    tiny = _new(L, 2, ksize=2)
    L.sourmash_err_clear()
    assert L.smh_add_protein(tiny, REC50, len(REC50)) == 1    # W == 0: add_sequence's panic
    L.sourmash_err_clear()
    for p in (dna, tiny):
        L.kmerminhash_free(p)


def test_without_a_device_nothing_is_applied(pkg_lib):
    L = pkg_lib
    off = (C.c_uint64 * 2)(0, len(REC50))
    for mol in (1, 2, 3):
        p = _new(L, mol, num=1000, max_hash=0)
        L.kmerminhash_add_hash(p, 7)
        rcs = (L.smh_add_protein(p, REC50, len(REC50)), L.smh_add_proteins(p, REC50, off, 1))
        if L.smh_device_available():
            assert rcs == (0, 0) and L.kmerminhash_get_mins_size(p) == 1 + KNOWN[(ar.ALPHABETS[mol - 1], 27)][0]
        else:
            assert rcs == (2, 2) and L.kmerminhash_get_mins_size(p) == 1 and L.kmerminhash_get_min_idx(p, 0) == 7
        L.sourmash_err_clear()
        L.kmerminhash_free(p)


def test_geometry_is_reported(pkg_lib):
    t, r = C.c_uint32(), C.c_uint32()
    pkg_lib.smh_amino_geometry(1 << 20, 9, C.byref(t), C.byref(r))
    assert t.value > 0 and r.value > 0 and t.value % r.value == 0
    one = (t.value, r.value)
    for total, win in ((100, 7), (1 << 30, 16), (5000, 42), (5000, 64)):      # one geometry for every tiled launch
        pkg_lib.smh_amino_geometry(total, win, C.byref(t), C.byref(r))
        assert (t.value, r.value) == one
