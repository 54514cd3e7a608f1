"""The nearest neighbours of a batch restated in plain Python (the rules of include/sourmash_amd.h, smh_index_nearest_many;
DESIGN.md 3.23).

No product import: this is what the device kernels are compared against, row for row.

The rows of a query are those of search_many_restatement.search_many under the same metric, threshold and threshold_common,
ordered by the metric's value DESCENDING -- the value is ONE float division, so two fractions that round to the same double
tie -- then by node ASCENDING; the first k of them.  A row is the tuple (node, common, node_size, query_size)."""
import search_many_restatement as SR

MAX_K = 256                    # smh_nearest_geometry's first value


def order(rows, metric):
    return sorted(rows, key=lambda r: (-SR.value(metric, r[1], r[3], r[2]), r[0]))


def select(shared_rows, k, metric, threshold, threshold_common=0):
    """nearest from the rows SR.shared computed once (every metric and threshold selects among them)"""
    return [order(rows, metric)[:k] for rows in SR.select(shared_rows, metric, threshold, threshold_common)]


def nearest(sketches, queries, k, metric, threshold, threshold_common=0):
    return [order(rows, metric)[:k] for rows in SR.search_many(sketches, queries, metric, threshold, threshold_common)]


def nearest_self(sketches, k, metric, threshold, threshold_common=0):
    """the sketches against themselves, the rows node == query left out (they take none of the k places)"""
    return [order(rows, metric)[:k] for rows in SR.search_self(sketches, metric, threshold, threshold_common, upper_only=False)]
