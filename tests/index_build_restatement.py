"""Building an index from records and concatenating indexes, restated in plain Python (the rules of include/sourmash_amd.h,
"Building an index from records").  No product import, no numpy: match_restatement.window_hashes for DNA,
amino_restatement's sketches for the translated and the amino-acid arms, dicts and sorted().

  node g       the records r with groups[r] == g (groups None: record r alone), in order
  DNA          every valid window's hash (match's rule: a window holding a byte outside ACGTacgt is skipped) that is
               <= max_hash, distinct and ascending as unsigned 64-bit; with abundances the number of windows that have it
  other arms   what a fresh oracle sketch of like's parameters holds after the group's records (translated, or amino input)
  result       CSR: offsets (n_groups + 1, from 0), hashes, abundances or None
  refusals     Refused, in the order the header lists them; a count of 2^32 or more names the lowest group"""
import amino_restatement
import match_restatement

Refused = match_restatement.Refused
U64_MAX = (1 << 64) - 1
MAX_GROUPS = 1 << 24
MAX_PAIRS = (1 << 31) - 1
NUCLEOTIDE, AMINO = 0, 1


def check(like, input_kind, records, groups, n_groups, offsets=None, total_len=None):
    """like: dict(num, ksize, molecule, seed, max_hash, track) or None.  offsets / total_len: only to restate their refusals
    (records given as a list of bytes always ascend)"""
    if like is None:
        raise Refused("like is NULL")
    if records is None:
        raise Refused("seq / offsets is NULL")
    if input_kind not in (NUCLEOTIDE, AMINO):
        raise Refused("unknown input %r" % (input_kind,))
    if not (like["num"] == 0 and like["max_hash"] != 0):
        raise Refused("like is not a scaled sketch")
    if input_kind == AMINO and like["molecule"] == "DNA":
        raise Refused("amino-acid input needs a protein, dayhoff or hp sketch")
    if offsets is not None:
        for r in range(len(offsets) - 1):
            if offsets[r + 1] < offsets[r]:
                raise Refused("offsets must ascend (record %d)" % r)
        if total_len is not None and len(offsets) > 1 and offsets[-1] > total_len:
            raise Refused("the last offset lies beyond the batch")
    if groups is not None:
        for r, g in enumerate(groups):
            if g >= n_groups:
                raise Refused("groups[%d] is %d; there are %d groups" % (r, g, n_groups))
    elif n_groups != len(records):
        raise Refused("groups is NULL but n_groups differs from the number of records")
    window = like["ksize"] if like["molecule"] == "DNA" else like["ksize"] // 3
    if window == 0:
        raise Refused("window size must be non-zero")
    if n_groups >= MAX_GROUPS:
        raise Refused("n_groups is %d; a call builds fewer than 2^24 nodes" % n_groups)


def node_counts(records, like, input_kind=NUCLEOTIDE):
    """hash -> count over the windows of `records` (one group's), sampled at like's max_hash"""
    counts = {}
    if like["molecule"] == "DNA":
        for rec in records:
            for h in match_restatement.window_hashes(rec, like["ksize"], like["seed"]):
                if h <= like["max_hash"]:
                    counts[h] = counts.get(h, 0) + 1
        return counts
    fn = amino_restatement.amino_sketch if input_kind == AMINO else amino_restatement.translated_sketch
    mh = fn(records, like["molecule"], like["ksize"], 0, like["max_hash"], True, like["seed"])
    return dict(zip(mh.mins, mh.abunds))


def narrow(counts_per_group):
    """the 32-bit rule: 2^32 - 1 is kept, 2^32 refused naming the lowest group"""
    for g, counts in enumerate(counts_per_group):
        if any(c >> 32 for c in counts.values()):
            raise Refused("group %d holds a hash seen in 2^32 or more windows" % g)


def csr(counts_per_group, track):
    """(offsets, hashes, abunds | None) of per-group hash -> count dicts: hashes ascending as unsigned 64-bit"""
    if track:
        narrow(counts_per_group)
    offsets, hashes, abunds = [0], [], []
    for counts in counts_per_group:
        for h in sorted(counts):
            hashes.append(h)
            abunds.append(counts[h])
        offsets.append(len(hashes))
    if len(hashes) > MAX_PAIRS:
        raise Refused("more than 2^31 - 1 (group, hash) pairs")
    return offsets, hashes, abunds if track else None


def build(records, groups, n_groups, like, input_kind=NUCLEOTIDE):
    """-> (offsets, hashes, abunds | None).  records: a list of bytes; groups: a list of ints or None"""
    check(like, input_kind, records, groups, n_groups)
    members = [[] for _ in range(n_groups)]
    for r, rec in enumerate(records):
        members[r if groups is None else groups[r]].append(rec)
    return csr([node_counts(m, like, input_kind) for m in members], like["track"])


def concat(parts):
    """parts: (offsets, hashes, abunds | None) each, or None for a NULL part -> the same triple; abundances are kept iff every
    part has them (no part: kept, over nothing)"""
    if parts is None:
        raise Refused("parts is NULL")
    offsets, hashes, abunds = [0], [], []
    keep = all(p is not None and p[2] is not None for p in parts)
    nodes = 0
    for k, p in enumerate(parts):
        if p is None:
            raise Refused("parts[%d] is NULL" % k)
        off, hs, ab = p
        nodes += len(off) - 1
        for v in range(len(off) - 1):   # (a part's offsets need not start at 0; its hashes are those between them)
            offsets.append(offsets[-1] + off[v + 1] - off[v])
        hashes.extend(hs[:off[-1] - off[0]])
        if keep:
            abunds.extend(ab[:off[-1] - off[0]])
    if nodes > (1 << 32) - 2:
        raise Refused("more than 2^32 - 2 nodes")
    return offsets, hashes, abunds if keep else None
