"""The restatement of the signature-scan rules (tests/sigscan_restatement.py) checked against things it does not define:
Python's json on the fixture files, and the two regular expressions that pin CLOSED and OPEN.  Needs no GPU and no library."""
import itertools
import json

import sigscan_restatement as R


def _number_arrays(doc):
    """the `mins` and `abundances` arrays of a parsed document in the order they are written (abundances behind mins)"""
    out = []
    for sig in doc:
        for sk in sig["signatures"]:
            keys = [k for k in sk if k in ("mins", "abundances")]          # (dict order is file order)
            out.extend(sk[k] for k in keys if sk[k] is not None)
    return out


def test_fixture_tokens_are_the_arrays_python_json_reads():
    texts = R.fixture_texts()
    assert len(texts) == 8
    for text in texts:
        skeleton, spans, values = R.scan(text)
        filled = [values[s["first_token"]:s["first_token"] + s["n_tokens"]] for s in spans if s["n_tokens"]]
        want = [a for a in _number_arrays(json.loads(text)) if a]
        assert filled == want
        assert all(s["status"] == R.CLOSED and s["bad_off"] == R.NONE for s in spans)
        assert sum(s["n_tokens"] for s in spans) == len(values)


def test_fixture_skeletons_parse_as_json_and_are_small():
    for path, text in zip(R.fixture_paths(), R.fixture_texts()):
        skeleton, spans, _ = R.scan(text)
        assert len(skeleton) + sum(s["end"] - s["start"] for s in spans) == len(text)
        doc, full = json.loads(skeleton), json.loads(text)
        assert len(doc) == len(full)
        for a, b in zip(doc, full):
            assert {k: v for k, v in a.items() if k != "signatures"} == {k: v for k, v in b.items() if k != "signatures"}
            for x, y in zip(a["signatures"], b["signatures"]):
                assert x["mins"] == [] and {k: v for k, v in x.items() if k not in ("mins", "abundances")} == \
                    {k: v for k, v in y.items() if k not in ("mins", "abundances")}
        if path.endswith("genome-s10+s11.sig"):
            assert (len(text), len(skeleton)) == (77044, 1317)


def test_every_status_on_crafted_spans():
    for text, want in R.STATUS_SPANS:
        _, spans, values = R.scan(text)
        assert spans[0]["status"] == want, (text[:40], spans[0])
        assert (spans[0]["bad_off"] == R.NONE) == (want in (R.CLOSED, R.OPEN))
    _, spans, values = R.scan(b"[1,,2]")
    assert spans[0]["bad_off"] == 3 and values == [1, 2]
    _, spans, values = R.scan(b"[1 2]")
    assert spans[0]["bad_off"] == 3
    _, spans, values = R.scan(b"[5,01]")
    assert spans[0]["bad_off"] == 3 and values == [5, 0]
    _, spans, values = R.scan(b"[7,18446744073709551616,18446744073709551615]")
    assert (spans[0]["status"], spans[0]["bad_off"], values) == (R.OVERFLOW, 3, [7, 0, 2 ** 64 - 1])
    _, spans, values = R.scan(b"[99999999999999999999,,1]")          # the lowest rule decides, not the lowest byte
    assert (spans[0]["status"], spans[0]["bad_off"]) == (R.BAD_SYNTAX, 22)
    skeleton, spans, values = R.scan(b'{"a":[1,-2],"b":[1.5],"c":[1e3]}')
    assert skeleton == b'{"a":[-2],"b":[.5],"c":[e3]}' and values == [1, 1, 1]
    assert [s["status"] for s in spans] == [R.OPEN, R.CLOSED, R.CLOSED]


def test_the_pin_on_every_short_span():
    """every span of up to six bytes over an alphabet that reaches each rule, and the crafted ones"""
    for n in range(7):
        for combo in itertools.product(b"0 1,\n9", repeat=n):
            assert R.pin_holds(bytes(combo)), bytes(combo)
    for text, _ in R.STATUS_SPANS:
        _, spans, _ = R.scan(text)
        assert R.pin_holds(text[spans[0]["start"]:spans[0]["end"]]), text[:40]


def test_strings_hide_brackets_and_escapes_count():
    skeleton, spans, values = R.scan(b'{"n":"[1,2,3]","m":[4,5]}')
    assert values == [4, 5] and skeleton == b'{"n":"[1,2,3]","m":[]}'
    for name in R.DECOY_NAMES:
        text = b'{"name":' + name + b',"mins":[6,7]}'
        skeleton, spans, values = R.scan(text)
        assert values == [6, 7] and len(spans) == 1 and json.loads(skeleton)["name"] == json.loads(name)
    # an even run of backslashes in front of a quote ends the string, an odd one does not
    assert R.scan(b'"a\\\\"[1]')[2] == [1] and R.scan(b'"a\\\\\\"[1]')[2] == []
    # a span that runs to the end of the text
    _, spans, values = R.scan(b"[1, 2,")
    assert (spans[0]["end"], spans[0]["status"], values) == (6, R.OPEN, [1, 2])
