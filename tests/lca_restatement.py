"""Taxonomic LCA on an index, restated in plain Python (the rules of include/sourmash_amd.h, "Taxonomic LCA"; DESIGN.md
3.15).  No product import, no numpy: sets, dicts, Counter, and match_restatement.window_hashes for the records.

  taxonomy       parent[t] for every taxon, taxon 0 the root; node_taxon[i] per node, NO_TAXON = no lineage
  lca(a, b)      the deepest common ancestor, from the two ancestor sets; NO_TAXON is the identity
  hash taxon     lca over the taxa of the nodes holding the hash; NO_TAXON when none has one; assigned = held and not NO_TAXON
  counts         Counter of the taxa of a query's assigned hashes, as (taxon, count) ascending
  find_lca       the LITERAL rule: a tree of nested dicts built from the root paths, descended while there is one child
  join           the fold of that rule on summaries (x, f): what the device's wave reduction computes"""
import collections

import match_restatement as M

NO_TAXON = 0xFFFFFFFF
NONE, FOUND, DISAGREE = 0, 1, 2


def root_path(parent, t):
    """[root, ..., t]"""
    path = [t]
    while t != 0:
        t = parent[t]
        path.append(t)
    return path[::-1]


def depth(parent, t):
    return len(root_path(parent, t)) - 1


def lca(parent, a, b):
    if a == NO_TAXON:
        return b
    if b == NO_TAXON:
        return a
    common = set(root_path(parent, a)) & set(root_path(parent, b))
    return max(common, key=lambda t: depth(parent, t))


def owners_of(nodes):
    """hash -> the nodes holding it"""
    return M.owners_of(nodes)


def hash_taxon(parent, node_taxon, owners, h):
    t = NO_TAXON
    for node in owners.get(h, ()):
        t = lca(parent, t, node_taxon[node])
    return t


def counts(parent, node_taxon, owners, query):
    """-> ([(taxon, count), ...] taxon ascending, [taxon or NO_TAXON per query hash in ascending hash order])"""
    per = [hash_taxon(parent, node_taxon, owners, h) for h in sorted(set(int(x) for x in query))]
    c = collections.Counter(t for t in per if t != NO_TAXON)
    return sorted(c.items()), per


def find_lca(parent, taxa):
    """the literal rule -> (taxon, status)"""
    tree = {}
    for t in taxa:
        node = tree
        for step in root_path(parent, t):
            node = node.setdefault(step, {})
    if not tree:
        return NO_TAXON, NONE
    at, below = 0, tree[0]
    while len(below) == 1:
        (at, below), = below.items()
    return at, DISAGREE if below else FOUND


def join(parent, a, b):
    """summaries (x, f), None = the empty set"""
    if a is None:
        return b
    if b is None:
        return a
    (x, fx), (y, fy) = a, b
    if depth(parent, x) > depth(parent, y):
        (x, fx), (y, fy) = (y, fy), (x, fx)
    l = lca(parent, x, y)
    if l != x:
        return l, True
    if x == y:
        return x, fx or fy
    return (x, True) if fx else (y, fy)


def status_of(summary):
    if summary is None:
        return NO_TAXON, NONE
    return summary[0], DISAGREE if summary[1] else FOUND


def rollup(parent, pairs):
    """counts added to all ancestors: dict taxon -> count"""
    out = collections.Counter()
    for t, c in pairs:
        for step in root_path(parent, t):
            out[step] += c
    return dict(out)


def classify_counts(parent, pairs, threshold):
    return find_lca(parent, [t for t, c in pairs if c >= threshold])


def classify_record(parent, node_taxon, owners, seq, ksize, seed, max_hash):
    """-> (windows, distinct, hit_distinct, assigned_distinct, taxon, status)"""
    sampled = [h for h in M.window_hashes(seq, ksize, seed) if h <= max_hash]
    hits = set(h for h in sampled if h in owners)
    taxa = [hash_taxon(parent, node_taxon, owners, h) for h in hits]
    taxa = [t for t in taxa if t != NO_TAXON]
    return (len(sampled), len(set(sampled)), len(hits), len(taxa)) + find_lca(parent, taxa)


def classify_records(parent, node_taxon, nodes, records, ksize, seed, max_hash):
    owners = nodes if isinstance(nodes, dict) else owners_of(nodes)
    return [classify_record(parent, node_taxon, owners, r, ksize, seed, max_hash) for r in records]
