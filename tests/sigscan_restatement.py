"""The rules by which signature JSON text is cut into number spans, values and a skeleton (include/sourmash_amd.h, "Signature
JSON on the device"), restated as plain Python.  This file is normative: the device kernels, the shared C++
core (sourmash-rust_amd/csrc/sigscan_core.hpp) and its serial driver are tested against it, never the other way round.

Every rule is written here the long way -- a list of flags per byte, slices, regular expressions -- and not as the automaton
the C++ uses, so that the two are independent statements of the same thing.

    scan(text) -> (skeleton, spans, values)
        skeleton   bytes: the text with every span's bytes removed
        spans      one dict per '[' outside a string, in order: start, end (the span is text[start:end]), first_token, n_tokens,
                   status, bad_off (NONE: no offending byte)
        values     every token of every span as an int, in document order; a token that breaks a rule is 0

A plain module, not a conftest: nothing here changes how tests are collected."""
import glob
import json
import os
import random
import re

CLOSED, OPEN, OVERFLOW, BAD_SYNTAX = 0, 1, 2, 3
NONE = 2 ** 64 - 1
U64_MAX = 2 ** 64 - 1
BLANKS = b" \n\t\r"
SPAN_BYTES = b"0123456789," + BLANKS
DIGITS = b"0123456789"

# The CPU pin: a span whose tokens all fit 64 bits is CLOSED or OPEN exactly when these say so.
_TOKEN = rb"(?:0|[1-9][0-9]*)"
_B = rb"[ \n\t\r]*"
CLOSED_RE = re.compile(rb"\A" + _B + rb"(?:" + _TOKEN + _B + rb"(?:," + _B + _TOKEN + _B + rb")*)?\Z")
OPEN_RE = re.compile(rb"\A" + _B + rb"(?:" + _TOKEN + _B + rb"," + _B + rb")+\Z")


def inside_string(text):
    """inside[i]: an odd number of unescaped '"' precede byte i.  A '"' is escaped if it is directly preceded by an odd-length
    run of backslashes."""
    inside = bytearray(len(text))                 # (only the quotes are visited: the texts of the tests are megabytes long)
    opened = None                                 # the unescaped quote that an odd count stands behind
    at = text.find(b'"')
    while at != -1:
        run = 0
        while at - run - 1 >= 0 and text[at - run - 1] == 0x5C:
            run += 1
        if run % 2 == 0:
            if opened is None:
                opened = at
            else:
                inside[opened + 1:at + 1] = b"\x01" * (at - opened)
                opened = None
        at = text.find(b'"', at + 1)
    if opened is not None:
        inside[opened + 1:] = b"\x01" * (len(text) - opened - 1)
    return inside


def span_status(span, base=0):
    """(status, bad_off) of a span's bytes; base: the text offset of span[0]"""
    bad_syntax, overflow = [], []
    prev = None                                   # the previous non-blank byte of the span
    for j, c in enumerate(span):
        if c in BLANKS:
            continue
        digit = c in DIGITS
        starts_token = digit and (j == 0 or span[j - 1] not in DIGITS)
        if c == 0x2C and (prev is None or prev not in DIGITS):
            bad_syntax.append(j)                  # a comma whose previous non-blank byte is not a digit
        if starts_token:
            if prev is not None and prev in DIGITS:
                bad_syntax.append(j)              # a token whose previous non-blank byte is a digit
            token = re.match(rb"[0-9]+", span[j:]).group()
            if len(token) > 1 and token[0] == 0x30:
                bad_syntax.append(j)              # more than one digit, starting with 0
            elif int(token) > U64_MAX:
                overflow.append(j)
        prev = c
    if bad_syntax:
        return BAD_SYNTAX, base + min(bad_syntax)
    if overflow:
        return OVERFLOW, base + min(overflow)
    return (OPEN if prev == 0x2C else CLOSED), NONE


def token_value(token):
    if len(token) > 1 and token[0] == 0x30:
        return 0
    v = int(token)
    return v if v <= U64_MAX else 0


def scan(text):
    text = bytes(text)
    inside = inside_string(text)
    skeleton, spans, values = bytearray(), [], []
    run_of_span_bytes = re.compile(rb"[0-9, \n\t\r]*")
    i = 0
    while i < len(text):
        at = text.find(b"[", i)                   # every byte up to the next '[' is kept as it is
        if at == -1:
            skeleton += text[i:]
            break
        skeleton += text[i:at + 1]
        i = at + 1
        if inside[at]:
            continue
        end = run_of_span_bytes.match(text, i).end()
        span = text[i:end]
        tokens = re.findall(rb"[0-9]+", span)
        status, bad = span_status(span, i)
        spans.append({"start": i, "end": end, "first_token": len(values), "n_tokens": len(tokens), "status": status, "bad_off": bad})
        values.extend(token_value(t) for t in tokens)
        i = end
    return bytes(skeleton), spans, values


def pin_holds(span):
    """the CPU pin for one span: with every token in range, CLOSED / OPEN exactly when the regular expressions say so"""
    status, _ = span_status(span)
    in_range = all(int(t) <= U64_MAX for t in re.findall(rb"[0-9]+", span))
    closed, opened = bool(CLOSED_RE.match(span)), bool(OPEN_RE.match(span))
    if not in_range:
        return status in (OVERFLOW, BAD_SYNTAX) and (status == BAD_SYNTAX) == (not (closed or opened))
    return (status == CLOSED) == closed and (status == OPEN) == opened and (status == BAD_SYNTAX) == (not (closed or opened))


# ---------------------------------------------------------------------------------------------------------------------------
# inputs shared by the tests

def fixture_paths():
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    return sorted(glob.glob(os.path.join(here, "*.sig")) + glob.glob(os.path.join(here, "sbt_v5", "*.sig")))


def fixture_texts():
    return [open(p, "rb").read() for p in fixture_paths()]


def sketch_json(mins, abundances=None, num=0, ksize=21, seed=42, max_hash=U64_MAX // 10, molecule="DNA", mins_text=None,
                abund_text=None):
    """one sketch object; mins_text / abund_text: the array written by hand (bytes)"""
    body = '{"num":%d,"ksize":%d,"seed":%d,"max_hash":%d,"mins":' % (num, ksize, seed, max_hash)
    body = body.encode() + (mins_text if mins_text is not None else json.dumps(list(mins), separators=(",", ":")).encode())
    body += b',"md5sum":"0123456789abcdef0123456789abcdef"'
    if abundances is not None or abund_text is not None:
        body += b',"abundances":' + (abund_text if abund_text is not None else
                                     (b"null" if abundances == "null" else json.dumps(list(abundances), separators=(",", ":")).encode()))
    return body + b',"molecule":"' + molecule.encode() + b'"}'


def signature_json(sketches, name=b'"a name"', filename=b'"a.fa"', extra=b""):
    """one signature object around sketch objects (bytes); name / filename are JSON values as written"""
    return (b'{"class":"sourmash_signature","email":"","hash_function":"0.murmur64","filename":' + filename + b',"name":' + name +
            b',"license":"CC0",' + extra + b'"signatures":[' + b",".join(sketches) + b'],"version":0.4}')


def document(signatures):
    return b"[" + b",".join(signatures) + b"]"


# (what the array of an ignored field and of `mins` looks like, what should happen) -- the statuses of the issue's list
STATUS_SPANS = [
    (b"[,1]", BAD_SYNTAX), (b"[1,,2]", BAD_SYNTAX), (b"[1 2]", BAD_SYNTAX), (b"[1,]", OPEN), (b"[01]", BAD_SYNTAX), (b"[00]", BAD_SYNTAX),
    (b"[0]", CLOSED), (b"[]", CLOSED), (b"[ \n\t\r]", CLOSED), (b"[1,-2]", OPEN), (b"[1.5]", CLOSED), (b"[1e3]", CLOSED),
    (b"[18446744073709551616]", OVERFLOW), (b"[184467440737095516150]", OVERFLOW), (b"[" + b"7" * 1000 + b"]", OVERFLOW),
    (b"[18446744073709551615]", CLOSED), (b"[ 1 , 2 ]", CLOSED), (b"[1 ,\n2,\t3\r]", CLOSED), (b"[1, 2 3]", BAD_SYNTAX), (b"[ , ]", BAD_SYNTAX),
    (b"[0,0]", CLOSED), (b"[10,0 ,007]", BAD_SYNTAX), (b"[99999999999999999999,01]", BAD_SYNTAX), (b"[1,[2],3]", OPEN),
]

DECOY_NAMES = [b'"[1,2,3]"', b'"\\"mins\\":["', b'"a\\"b"', b'"back\\\\"', b'"\\u005b1,2"', b'"\\\\\\"[7"', b'"]"', b'"[["']


def status_documents():
    """every status span as an ignored field of a signature and as `mins` itself: (name, text)"""
    out = []
    for k, (span, _) in enumerate(STATUS_SPANS):
        out.append(("ignored_%d" % k, document([signature_json([sketch_json([1, 2, 3])], extra=b'"unknown":' + span + b",")])))
        out.append(("mins_%d" % k, document([signature_json([sketch_json([], mins_text=span)])])))
        out.append(("abund_%d" % k, document([signature_json([sketch_json([5], abund_text=span)])])))
    return out


def crafted_documents():
    """(name, text) of single documents: accepted and refused ones, every one small"""
    docs = list(status_documents())
    for k, nm in enumerate(DECOY_NAMES):
        docs.append(("decoy_%d" % k, document([signature_json([sketch_json([3, 4, 9], [1, 1, 2])], name=nm, filename=nm)])))
    sk = sketch_json([1, 2, 3])
    docs += [
        ("empty_document", b"[]"), ("blank_document", b" [ ] \n"), ("empty_text", b""), ("no_sketches", document([signature_json([])])),
        ("two_signatures", document([signature_json([sk, sketch_json([7], ksize=31, molecule="protein")]), signature_json([sk], name=b"null")])),
        ("null_abundances", document([signature_json([sketch_json([1, 2], "null")])])),
        ("abund_other_length", document([signature_json([sketch_json([1, 2, 3], [4])])])),
        ("num_sketch", document([signature_json([sketch_json([9, 8], num=500, max_hash=0)])])),
        ("q9", document([signature_json([sketch_json([9], num=500, max_hash=77)])])),
        ("hp", document([signature_json([sketch_json([9], molecule="hp")]), signature_json([sketch_json([1], molecule="whatever")])])),
        ("not_an_array", b'{"a":[1,2]}'), ("number_document", b"12"), ("numbers_document", b"[1,2]"), ("trailing", b"[] x"),
        ("unclosed", b"[" + signature_json([sk])), ("unclosed_mins", document([signature_json([sk])])[:120]),
        ("cut_in_string", document([signature_json([sk])])[:60]), ("sketch_is_number", document([signature_json([b"5"])])),
        ("sketch_is_number_2", document([signature_json([sk, b"5"])])), ("missing_mins", document([signature_json([sk.replace(b'"mins"', b'"mims"')])])),
        ("mins_is_string", document([signature_json([sk.replace(b"[1,2,3]", b'"1"')])])), ("mins_nested", document([signature_json([sk.replace(b"[1,2,3]", b"[1,[2]]")])])),
        ("mins_with_string", document([signature_json([sk.replace(b"[1,2,3]", b'[1,"2"]')])])), ("mins_negative", document([signature_json([sk.replace(b"[1,2,3]", b"[1,-2]")])])),
        ("mins_float", document([signature_json([sk.replace(b"[1,2,3]", b"[1,2.0]")])])), ("mins_true", document([signature_json([sk.replace(b"[1,2,3]", b"[1,true]")])])),
        ("version_int", document([signature_json([sk]).replace(b'"version":0.4', b'"version":1')])), ("version_bad", document([signature_json([sk]).replace(b'"version":0.4', b'"version":"x"')])),
        ("backslash_outside", document([signature_json([sk])]).replace(b'"license"', b'\\"license"')), ("bracket_in_key", document([signature_json([sk], extra=b'"k[1,2]":[3],')])),
        ("nested_ignored", document([signature_json([sk], extra=b'"deep":[[1,2],[3,[4,5]],[]],')])), ("objects_in_array", document([signature_json([sk], extra=b'"o":[{"a":[1]},{"b":[2,3]}],')])),
        ("deep_array", document([signature_json([sk], extra=b'"d":' + b"[" * 125 + b"1" + b"]" * 125 + b",")])),
        ("too_deep_array", document([signature_json([sk], extra=b'"d":' + b"[" * 126 + b"1" + b"]" * 126 + b",")])),
        ("deep_empty", document([signature_json([sk], extra=b'"d":' + b"[" * 126 + b"]" * 126 + b",")])),
        ("float_exp", document([signature_json([sk], extra=b'"f":[1E5],')])), ("float_after_blank", document([signature_json([sk], extra=b'"f":[1 .5],')])),
        ("minus_glued", document([signature_json([sk], extra=b'"f":[1-2],')])), ("letters_glued", document([signature_json([sk], extra=b'"f":[1,2true],')])),
        ("true_after_comma", document([signature_json([sk], extra=b'"f":[1,true],')])), ("seed_overflow", document([signature_json([sk.replace(b'"seed":42', b'"seed":18446744073709551616')])])),
        ("ksize_big", document([signature_json([sk.replace(b'"ksize":21', b'"ksize":4294967296')])])), ("duplicate_mins", document([signature_json([sk.replace(b',"md5sum"', b',"mins":[4,5],"md5sum"')])])),
    ]
    return docs


def mutants(n=2000, seed=20):
    """byte-level mutants of small valid documents (the fixtures cut down to a few numbers per array, and crafted ones): a
    byte replaced by one that matters to the rules, removed, or doubled"""
    rng = random.Random(seed)
    pool = [t for _, t in crafted_documents() if t]
    for text in fixture_texts():
        pool.append(re.sub(rb"\[(\d+,\d+,\d+)[0-9,]*\]", rb"[\1]", text))
    alphabet = b'[],"\\ \n0179.eE-:{}tn'
    out = []
    for k in range(n):
        t = bytearray(pool[k % len(pool)])
        for _ in range(rng.choice((1, 1, 2, 3))):
            at = rng.randrange(len(t))
            how = rng.randrange(3)
            if how == 0:
                t[at] = rng.choice(alphabet)
            elif how == 1:
                del t[at]
            else:
                t.insert(at, rng.choice(alphabet))
            if not t:
                t = bytearray(b"[")
        out.append(bytes(t))
    return out
