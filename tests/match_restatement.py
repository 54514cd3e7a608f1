"""Matching records against an index, restated in plain Python (the rules of include/sourmash_amd.h, "Matching records";
DESIGN.md 3.13).  No product import, no numpy: pyoracle.hash_murmur and revcomp, loops, dicts and sets.

  window       a start p of record r with p + ksize <= len(r); skipped when it holds a byte outside ACGTacgt
  hash         murmur64 of the smaller of the upper-cased k-mer and its reverse complement
  sampled      hash <= max_hash (Python ints: unsigned, inclusive)
  hit          a sampled window whose hash some node holds
  row          (windows, distinct, hit_windows, hit_distinct, best, best_common); best = the node holding the most of the
               record's distinct hit hashes, the lowest index on ties, MISS without a hit
  hit list     per record its distinct hit hashes ascending, as CSR offsets + one flat list"""
import pyoracle

MISS = 0xFFFFFFFF
U64_MAX = (1 << 64) - 1
_DNA = frozenset(b"ACGTacgt")
_UPPER = bytes.maketrans(b"acgt", b"ACGT")
_cache = {}


class Refused(Exception):
    """what the library reports as SOURMASH_ERROR_CODE_MSG (3)"""


def kmer_hash(kmer, seed=42):
    """hash of one valid window (bytes over ACGTacgt)"""
    up = bytes(kmer).translate(_UPPER)
    rc = pyoracle.revcomp(up)
    canon = up if up < rc else rc
    key = (canon, seed)
    h = _cache.get(key)
    if h is None:
        h = _cache[key] = pyoracle.hash_murmur(canon, seed)
    return h


def window_hashes(seq, ksize, seed=42):
    """the hashes of the record's valid windows, in window order"""
    seq = bytes(seq)
    out = []
    for p in range(len(seq) - ksize + 1):
        kmer = seq[p:p + ksize]
        if all(c in _DNA for c in kmer):
            out.append(kmer_hash(kmer, seed))
    return out


def check_index(node_params):
    """node_params: (molecule, num, ksize, seed, max_hash) per node -> (ksize, seed, max_hash) of node 0, or Refused"""
    if not node_params:
        raise Refused("no node")
    for mol, num, ksize, seed, mx in node_params:
        if mol != "DNA" or num != 0 or mx == 0 or (ksize, seed, mx) != tuple(node_params[0][2:]):
            raise Refused((mol, num, ksize, seed, mx))
    return tuple(node_params[0][2:])


def owners_of(nodes):
    """hash -> ascending list of the nodes holding it"""
    own = {}
    for i, node in enumerate(nodes):
        for h in set(int(x) for x in node):
            own.setdefault(h, []).append(i)
    return own


def match_record(seq, ksize, seed, max_hash, owners):
    """-> (row, ascending distinct hit hashes)"""
    sampled = [h for h in window_hashes(seq, ksize, seed) if h <= max_hash]
    hits = [h for h in sampled if h in owners]
    tally = {}
    for h in set(hits):
        for node in owners[h]:
            tally[node] = tally.get(node, 0) + 1
    best, best_common = MISS, 0
    for node in sorted(tally):
        if tally[node] > best_common:
            best, best_common = node, tally[node]
    return (len(sampled), len(set(sampled)), len(hits), len(set(hits)), best, best_common), sorted(set(hits))


def match(records, ksize, seed, max_hash, nodes):
    """-> (rows, hit_offsets, hit_hashes) for the records (bytes each) against the nodes (iterables of hashes)"""
    owners = nodes if isinstance(nodes, dict) else owners_of(nodes)
    rows, offsets, flat = [], [0], []
    for seq in records:
        row, hit = match_record(seq, ksize, seed, max_hash, owners)
        rows.append(row)
        flat.extend(hit)
        offsets.append(len(flat))
    return rows, offsets, flat
