"""The thresholded search of a batch restated in plain Python over sets (the rules of include/sourmash_amd.h,
smh_index_search_many).

No product import: this is what the device kernels are compared against, row for row.

    sketches          list of iterables of hashes (S_0 .. S_{n-1})
    queries           list of iterables of hashes
    metric            JACCARD, CONTAINMENT_NODE, CONTAINMENT_QUERY or MAX_CONTAINMENT
    threshold         a float; the comparison is strict
    threshold_common  0 is read as 1

Returns one list of rows per query; a row is the tuple (node, common, node_size, query_size), nodes ascending."""

JACCARD, CONTAINMENT_NODE, CONTAINMENT_QUERY, MAX_CONTAINMENT = 0, 1, 2, 3
METRICS = (JACCARD, CONTAINMENT_NODE, CONTAINMENT_QUERY, MAX_CONTAINMENT)
MAX_QUERIES = 65535            # queries per chunk: the second dimension of a grid
MAX_POSITIONS = 0xFFFFFFFF     # a chunk of several queries holds fewer positions than this


def value(metric, common, query_size, node_size):
    """one division of two integers converted to double (Python's float division of ints below 2^53 is exactly that)"""
    if metric == JACCARD:
        den = max(1, query_size + node_size - common)
    elif metric == CONTAINMENT_NODE:
        den = node_size
    elif metric == CONTAINMENT_QUERY:
        den = query_size
    elif metric == MAX_CONTAINMENT:
        den = min(query_size, node_size)
    else:
        raise ValueError("unknown metric")
    return float(common) / float(den)


def reported(metric, threshold, threshold_common, common, query_size, node_size):
    if common < max(1, threshold_common):
        return False                      # (a pair that shares nothing ends here: no division by an empty sketch)
    return value(metric, common, query_size, node_size) > threshold


def shared(sketches, queries):
    """per query the rows of every node that shares a hash with it, whatever its value is: the threshold only selects among
    these (lets one pass over a large case serve every metric and threshold)"""
    sets = [set(s) for s in sketches]
    out = []
    for q in queries:
        q = set(q)
        rows = []
        for i, s in enumerate(sets):
            common = len(q & s)
            if common:
                rows.append((i, common, len(s), len(q)))
        out.append(rows)
    return out


def select(shared_rows, metric, threshold, threshold_common=0):
    return [[r for r in rows if reported(metric, threshold, threshold_common, r[1], r[3], r[2])] for rows in shared_rows]


def search_many(sketches, queries, metric, threshold, threshold_common=0):
    return select(shared(sketches, queries), metric, threshold, threshold_common)


def search_self(sketches, metric, threshold, threshold_common=0, upper_only=False):
    """the sketches against themselves: search_many without the rows node == query, and with upper_only without node < query"""
    full = search_many(sketches, sketches, metric, threshold, threshold_common)
    return [[r for r in rows if (r[0] > q if upper_only else r[0] != q)] for q, rows in enumerate(full)]


def cut_chunks(sizes, n_nodes, budget):
    """[(first query, end)]: as many consecutive queries as the budget holds (query, node) counters for, one at least, at most
    MAX_QUERIES, and fewer than MAX_POSITIONS positions unless the chunk is a single query"""
    per = min(max(budget // max(n_nodes, 1), 1), MAX_QUERIES)
    out, a = [], 0
    while a < len(sizes):
        b = min(len(sizes), a + per)
        while b > a + 1 and sum(sizes[a:b]) >= MAX_POSITIONS:
            b -= 1
        out.append((a, b))
        a = b
    return out
