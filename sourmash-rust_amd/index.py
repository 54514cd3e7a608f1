"""Callers of the hot path in the reference's index layer, rebuilt on the block-compare kernels:

  LinearIndex.find          reference src/index/linear.rs:25-45 + src/index/search.rs:3-9
  most_common (scaffold)    reference src/index/sbt.rs:361-370 (nearest leaf = arg-max count_common)
  ResidentIndex.gather      the greedy decomposition of a query (no counterpart in the reference crate: the rules are those
                            of include/sourmash_amd.h, smh_index_gather)
  ResidentIndex.gather_many the same decomposition for a batch of queries in one device call (smh_index_gather_many)
  ResidentIndex.search_many the (query, node) pairs of a batch of queries over a threshold, as a sparse list (no counterpart
                            either: include/sourmash_amd.h, smh_index_search_many); pairwise is the index against itself
  ResidentIndex.nearest     of those pairs the best k per query, best first (smh_index_nearest_many); knn is the index against
                            itself: the k-nearest-neighbour graph
  ResidentIndex.cluster     the clusters of the index's own nodes under such a threshold, made on the device (no counterpart:
                            include/sourmash_amd.h, smh_index_cluster): connected components or greedy representatives
  ResidentIndex.collapse    one sketch per group of nodes -- union, core, prevalence -- as a new resident index made on the
                            device (no counterpart: include/sourmash_amd.h, "Collapsing an index by groups"); read / sketches
                            bring an index's own sketches back to the host (smh_index_read)
  ResidentIndex.from_records  an index built straight from records on the device, one group of records a node, and
                            ResidentIndex.concat, which joins resident indexes in HBM (no counterpart: include/sourmash_amd.h,
                            "Building an index from records")
  ResidentIndex.filter      the same nodes cut down to the hashes that pass a rule -- kept in / dropped from an operand sketch,
                            an abundance window, a window on the number of nodes that hold the hash -- as a new resident
                            index made on the device; subtract / intersect / inflate / flatten are spelled through it, and
                            select takes whole nodes in any order (no counterpart: include/sourmash_amd.h, "Filtering an
                            index")
  ResidentIndex.match       the k-mers of every record of a batch the index knows, and each record's best node (no counterpart
                            either: include/sourmash_amd.h, "Matching records")

A "node" here is a KmerMinHash (the reference's Leaf wraps a Signature whose first sketch is used,
src/index.rs:108-161)."""
import collections
import collections.abc
import ctypes as C
import math
import weakref

import numpy as np

from ._lib import SmhFilter, SmhGatherRow, SmhLcaRow, SmhMatchRow, SmhSearchRow, lib, u32p, u64p
from .errors import SourmashError, call

UNASSIGNED = 0xFFFFFFFF

GatherRecord = collections.namedtuple("GatherRecord", [
    "match", "common_remaining", "common_original", "size_match", "abund_sum",   # the integers of SmhGatherRow
    "f_orig_query",        # common_original / |query|
    "f_match",             # common_remaining / size_match
    "f_unique_to_query",   # common_remaining / |query|
    "f_unique_weighted",   # abund_sum / sum of all the query's abundances
    "average_abund",       # abund_sum / common_remaining
    "median_abund", "std_abund",   # numpy median / std over the abundances of the positions this row consumed
    "remaining_bp"])       # scaled * (query positions nobody has consumed after this row)
GatherResult = collections.namedtuple("GatherResult", ["rows", "assigned"])
AngularResult = collections.namedtuple("AngularResult", ["dot", "cosine", "angular"])
# one numpy array per field of SmhMatchRow (uint32, a record each); hit_offsets / hit_hashes (uint64) or None
MatchResult = collections.namedtuple("MatchResult", ["windows", "distinct", "hit_windows", "hit_distinct", "best", "best_common",
                                                     "hit_offsets", "hit_hashes"])
NO_MATCH = 0xFFFFFFFF
_MATCH_ROW = np.dtype([(name, np.uint32) for name, _ in SmhMatchRow._fields_])
# one numpy array per field of SmhLcaRow (uint32, a record each)
LcaRecords = collections.namedtuple("LcaRecords", ["windows", "distinct", "hit_distinct", "assigned_distinct", "taxon", "status"])
NO_TAXON = 0xFFFFFFFF
LCA_NONE, LCA_FOUND, LCA_DISAGREE = 0, 1, 2
_LCA_ROW = np.dtype([(name, np.uint32) for name, _ in SmhLcaRow._fields_])
# the metrics of search_many / pairwise (SMH_SEARCH_* of include/sourmash_amd.h); their names are SearchResult's float columns
SEARCH_METRICS = {"jaccard": 0, "containment_node": 1, "containment_query": 2, "max_containment": 3}
_SEARCH_ROW = np.dtype([(name, np.uint32) for name, _ in SmhSearchRow._fields_])


class SearchResult:
    """The pairs search_many / pairwise report.  offsets (uint64, queries + 1): the rows of query q are
    [offsets[q], offsets[q + 1]); node, common, node_size, query_size (uint32, a row each) are the device's integers, ordered
    by query, then node; jaccard, containment_node, containment_query and max_containment (float64, a row each) are derived
    here from the integers, one division each, as the rule of the header derives the value it thresholds.  Rows from nearest /
    nearest_block_dev / knn are ordered by query, then by the metric's value descending, then node."""

    def __init__(self, offsets, rows, ksize=None, molecule=None):
        self.offsets = offsets
        self.node, self.common, self.node_size, self.query_size = (rows[name] for name in _SEARCH_ROW.names)
        self.ksize, self.molecule = ksize, molecule
        c, ls, lq = (a.astype(np.float64) for a in (self.common, self.node_size, self.query_size))
        self.jaccard = c / np.maximum(1.0, lq + ls - c)
        self.containment_node = c / ls
        self.containment_query = c / lq
        self.max_containment = c / np.minimum(lq, ls)

    def __len__(self):
        return len(self.node)

    def rows_of(self, q):
        """the slice of query q's rows"""
        return slice(int(self.offsets[q]), int(self.offsets[q + 1]))

    def query(self):
        """the query of every row (uint32)"""
        return np.repeat(np.arange(len(self.offsets) - 1, dtype=np.uint32), np.diff(self.offsets).astype(np.int64))

    def ani(self, column="containment_query"):
        """value ** (1 / ksize) of a containment column: the point estimate of the average nucleotide identity that
        `sourmash --ani` prints.  DNA indexes only."""
        if column not in ("containment_node", "containment_query", "max_containment"):
            raise ValueError("ani is estimated from a containment column, not from %r" % (column,))
        if self.molecule != "DNA" or not self.ksize:
            raise ValueError("ani is defined for DNA sketches only (this result: %s)" % (self.molecule or "an index without nodes"))
        return getattr(self, column) ** (1.0 / self.ksize)


# the linkages of cluster (SMH_CLUSTER_* of include/sourmash_amd.h)
CLUSTER_LINKAGES = {"components": 0, "greedy": 1}


class Clustering:
    """What cluster reports.  cluster (uint32, a node each): the node's cluster, clusters numbered in ascending order of their
    smallest member; representative (uint32): the node that represents it; n_clusters; for the greedy linkage rep_common
    (uint32: the hashes a member shares with its representative, a representative's own size) and rep_value (float64: the
    metric's value of (node, representative), derived here from the integers with one division, as SearchResult derives its
    floats; 1.0 for a representative that holds a hash, NaN for an empty one) -- both None for components."""

    def __init__(self, cluster, representative, n_clusters, rep_common=None, sizes=None, metric=None):
        self.cluster, self.representative, self.n_clusters, self.rep_common = cluster, representative, int(n_clusters), rep_common
        self.rep_value = None
        if rep_common is not None:
            c, lv, lr = (a.astype(np.float64) for a in (rep_common, sizes, sizes[representative]))
            with np.errstate(invalid="ignore", divide="ignore"):
                self.rep_value = c / (lv + lr - c) if metric == "jaccard" else c / np.minimum(lv, lr)

    def __len__(self):
        return len(self.cluster)

    def sizes(self):
        """the nodes of every cluster (int64, n_clusters entries)"""
        return np.bincount(self.cluster, minlength=self.n_clusters)

    def members(self, c):
        """the nodes of cluster c, ascending"""
        return np.flatnonzero(self.cluster == c)


# the abundance modes of collapse (SMH_COLLAPSE_* of include/sourmash_amd.h) and the group of a node that takes no part
COLLAPSE_ABUNDS = {"flat": 0, "sum": 1, "count": 2}
COLLAPSE_DROP = 0xFFFFFFFF


# the operand modes and the abundances of the result of filter (SMH_FILTER_* of include/sourmash_amd.h)
FILTER_MODES = {None: 0, "keep": 1, "drop": 2}
FILTER_ABUNDS = {"own": 0, "flat": 1, "operand": 2}
FILTER_NO_MAX = 0xFFFFFFFF


class _OwnSketches(collections.abc.Sequence):
    """`nodes` of an index collapse() returned: its own sketches, read back from the device when one is first asked for (the
    length is known without that)."""

    def __init__(self, index):
        self._n = len(index)
        self._index = weakref.ref(index)   # (the index owns this object: a strong reference would make a cycle and delay its free)
        self._list = None

    def __len__(self):
        return self._n

    def __getitem__(self, k):
        if self._list is None:
            self._list = self._index().sketches()
        return self._list[k]


class _PartParams(collections.abc.Sequence):
    """(num, ksize, molecule, seed, max_hash, track) of every node of concat()'s result, taken from what its parts' nodes were
    when one is first asked for: a part contributes one tuple for all its nodes, an earlier concat()'s list, or its host
    sketches (kept alive here; the part's index itself may be freed) with the max_hash the part held them at."""

    def __init__(self, parts):
        self._sources, self._n, self._list = [], 0, None
        for p in parts:
            n = len(p)
            template, per_node = getattr(p, "_template", None), getattr(p, "_node_templates", None)
            if per_node is not None:
                self._sources.append(lambda per_node=per_node: list(per_node))
            elif template is not None:
                self._sources.append(lambda template=template, n=n: [template] * n)
            else:
                lo, hi = p.max_hash_range
                self._sources.append(lambda nodes=p.nodes, lo=lo, hi=hi: [
                    (m.num, m.ksize, m.molecule, m.seed, lo if lo == hi else m.max_hash, bool(m.track_abundance)) for m in nodes])
            self._n += n

    def __len__(self):
        return self._n

    def __getitem__(self, k):
        if self._list is None:
            self._list = [t for src in self._sources for t in src()]
            self._sources = None
        return self._list[k]


class _PickedParams(collections.abc.Sequence):
    """the per-node parameters of select()'s result: those of the parent's nodes ids[0], ids[1], ..."""

    def __init__(self, parent_params, ids):
        self._parent, self._ids = parent_params, [int(v) for v in ids]

    def __len__(self):
        return len(self._ids)

    def __getitem__(self, k):
        return self._parent[self._ids[k]]


def scaled_of_max_hash(max_hash):
    """the `scaled` a max_hash stands for: max_hash = 2^64 // scaled, so scaled = round(2^64 / max_hash)"""
    if max_hash <= 0:
        raise ValueError("not a scaled sketch: max_hash is 0")
    return max(1, ((1 << 64) + max_hash // 2) // max_hash)


def max_hash_of_scaled(scaled):
    """the max_hash a `scaled` stands for, min(2^64 // scaled, 2^64 - 1): the inverse of scaled_of_max_hash"""
    scaled = int(scaled)
    if scaled <= 0:
        raise ValueError("scaled must be positive")
    return min((1 << 64) // scaled, (1 << 64) - 1)


def lca_summarize(parent, taxa, counts):
    """The counts of lca_counts rolled up (`lca summarize`): dict taxon -> the sum of the counts of the taxon and of everything
    below it.  Host work on the small output: the device does not roll up."""
    out = collections.Counter()
    for t, c in zip(taxa, counts):
        t, c = int(t), int(c)
        while True:
            out[t] += c
            if t == 0:
                break
            t = int(parent[t])
    return dict(out)


def lca_classify(parent, taxa, counts, threshold=1):
    """(taxon, status) of the classification rule applied to the taxa with count >= threshold (`lca classify`): descend from
    the root through the union of their root paths while there is exactly one child; LCA_FOUND when nothing lies below where
    it stops, LCA_DISAGREE at a branching, (NO_TAXON, LCA_NONE) when no taxon reaches the threshold."""
    kept = {int(t) for t, c in zip(taxa, counts) if int(c) >= threshold}
    if not kept:
        return NO_TAXON, LCA_NONE
    children = {}
    for t in kept:
        while t != 0 and t not in children.get(int(parent[t]), ()):
            children.setdefault(int(parent[t]), set()).add(t)
            t = int(parent[t])
    at = 0
    while len(children.get(at, ())) == 1:
        (at,) = children[at]
    return at, LCA_DISAGREE if children.get(at) else LCA_FOUND


def _is_scaled(mh):
    return mh.num == 0 and mh.max_hash != 0


def _gather_result(query, rows, n_rows, assigned, scaled, abund_stats):
    """GatherResult of one query from the integers of the device (rows: n_rows SmhGatherRow; assigned: the query's
    positions): the derived floats of gather() and gather_many()."""
    nq = len(assigned)
    # a query without abundances weighs 1 per hash: its statistics are known without looking at it
    ab = query.abunds_np() if query.track_abundance and abund_stats and n_rows else None
    flat = not query.track_abundance
    total_ab = nq if flat else int(ab.sum(dtype=np.uint64)) if ab is not None else None
    out, left = [], nq
    if ab is not None:   # the positions of round r, for every r at once
        order = np.argsort(assigned, kind="stable")
        cuts = np.searchsorted(assigned[order], np.arange(n_rows + 1, dtype=np.uint32))
    for r in range(n_rows):
        w = rows[r]
        left -= w.common_remaining
        mine = ab[order[cuts[r]:cuts[r + 1]]] if ab is not None else None
        out.append(GatherRecord(
            w.match, w.common_remaining, w.common_original, w.size_match, w.abund_sum,
            w.common_original / nq, w.common_remaining / w.size_match, w.common_remaining / nq,
            w.abund_sum / total_ab if total_ab is not None else None,
            w.abund_sum / w.common_remaining,
            1.0 if flat else float(np.median(mine)) if ab is not None else None,
            0.0 if flat else float(np.std(mine)) if ab is not None else None,
            scaled * left))
    return GatherResult(out, assigned)


def search_minhashes(nodes, query, threshold):
    """indices i with nodes[i].similarity(query) > threshold"""
    return _find(nodes, query, threshold, False)


def search_minhashes_containment(nodes, query, threshold):
    """indices i with nodes[i].containment(query) > threshold"""
    return _find(nodes, query, threshold, True)


def _find(nodes, query, threshold, containment):
    n = len(nodes)
    arr = (C.c_void_p * max(n, 1))(*[m._p for m in nodes])
    out = (C.c_uint32 * max(n, 1))()
    cnt = C.c_uint32()
    call(lib().smh_find, arr, n, query._p, float(threshold), bool(containment), out, C.byref(cnt))
    return [int(out[i]) for i in range(cnt.value)]


class ResidentIndex:
    """Sketches copied once into HBM (additive ABI smh_index_*): repeated queries upload only the query.

    max_hash: build at that resolution from scaled nodes of mixed `scaled` (every node is cut on the device,
    smh_index_downsample).  `nodes` keeps the sketches as they were given: for an index built with max_hash, and for
    every index downsample() returns, they are the UNCUT sketches -- their max_hash and mins are not what the index holds
    (ask max_hash / max_hash_range, or cut a node with downsample_max_hash).

    The search calls take downsample=False.  With True both operands must be scaled sketches (else Msg): they meet at the
    smaller max_hash of the two, each finer side replaced by its cut -- a sketch by downsample_max_hash, an index by a child
    this index caches per max_hash (drop_downsampled() gives the children back).  Node positions in the results are those
    of this index: the cut never reorders."""

    def __init__(self, nodes, max_hash=None, *, _handle=None):
        self._L = lib()
        self.nodes = list(nodes)
        self._children = {}
        self._all_scaled = None
        self._h = _handle          # (None until a handle is owned: __del__ frees nothing else)
        if _handle is not None:
            return
        arr = (C.c_void_p * max(len(self.nodes), 1))(*[m._p for m in self.nodes])
        fine = call(self._L.smh_index_new, arr, len(self.nodes))
        if max_hash is None:
            self._h = fine
            return
        try:
            self._h = call(self._L.smh_index_downsample, fine, int(max_hash))   # a refusal leaves this object without a handle
        finally:
            self._L.smh_index_free(fine)

    def __del__(self):
        try:
            if self._h is not None:
                self._L.smh_index_free(self._h)
        except Exception:
            pass

    def __len__(self):
        return self._L.smh_index_len(self._h)

    def drop_dictionary(self):
        """gives back the dictionary an all-vs-all compare of the index with itself cached (smh_index_drop_dictionary)"""
        self._L.smh_index_drop_dictionary(self._h)

    # --- downsampling (additive ABI smh_index_downsample; the rules are in include/sourmash_amd.h)
    @property
    def max_hash_range(self):
        """(smallest, largest) max_hash over the nodes; (0, 0) for an empty index"""
        lo, hi = C.c_uint64(), C.c_uint64()
        call(self._L.smh_index_max_hash_range, self._h, C.byref(lo), C.byref(hi))
        return lo.value, hi.value

    @property
    def max_hash(self):
        """the max_hash every node has, or None when the nodes differ (or there are none)"""
        lo, hi = self.max_hash_range
        return lo if len(self) and lo == hi else None

    def downsample(self, max_hash=None, scaled=None):
        """This index cut at max_hash (or at the max_hash `scaled` stands for), made on the device from the resident
        arrays: a ResidentIndex of its own, cached here per max_hash.  Its `nodes` are this index's uncut sketches."""
        if (max_hash is None) == (scaled is None):
            raise ValueError("give max_hash or scaled")
        mx = int(max_hash) if max_hash is not None else max_hash_of_scaled(scaled)
        child = self._children.get(mx)
        if child is None:
            child = ResidentIndex(self.nodes, _handle=call(self._L.smh_index_downsample, self._h, mx))
            self._children[mx] = child
        return child

    def drop_downsampled(self):
        """gives back the cut indexes downsample() cached"""
        self._children.clear()

    def _scaled_range(self, what):
        """max_hash_range of an index whose nodes are all scaled sketches, else Msg"""
        if self._all_scaled is None:      # from the parameters the index was built with; its nodes never change
            self._all_scaled = bool(self._L.smh_index_all_scaled(self._h))
        if not self._all_scaled:
            raise SourmashError(3, "downsample: %s holds a node that is not a scaled sketch" % what)
        return self.max_hash_range

    def _at(self, common):
        lo, hi = self.max_hash_range
        return self if len(self) == 0 or lo == hi == common else self.downsample(max_hash=common)

    def _meet_sketch(self, query):
        """(index, query) at the smaller max_hash of the two"""
        if not _is_scaled(query):
            raise SourmashError(3, "downsample: the sketch is not a scaled sketch (num = %d, max_hash = %d)" % (query.num, query.max_hash))
        lo, _ = self._scaled_range("the index")
        qmx = query.max_hash
        common = min(qmx, lo) if len(self) else qmx
        return self._at(common), query if qmx == common else query.downsample_max_hash(common)

    def _meet_groups(self, queries):
        """the queries grouped by the index at which each meets this one: (index, positions in `queries`, the cut queries)"""
        met = [self._meet_sketch(q) for q in queries]
        groups = {}
        for k, (idx, _) in enumerate(met):
            groups.setdefault(id(idx), (idx, []))[1].append(k)
        for idx, members in groups.values():
            yield idx, members, [met[k][1] for k in members]

    def _meet_index(self, other):
        if other is self:
            lo, _ = self._scaled_range("the index")
            cut = self._at(lo)
            return cut, cut
        lo_a, _ = self._scaled_range("the row index")
        lo_b, _ = other._scaled_range("the column index")
        if len(self) == 0 or len(other) == 0:
            return self, other
        common = min(lo_a, lo_b)
        return self._at(common), other._at(common)

    def find(self, query, threshold, containment=False, downsample=False):
        if downsample:
            idx, q = self._meet_sketch(query)
            return idx.find(q, threshold, containment)
        out = (C.c_uint32 * max(len(self.nodes), 1))()
        cnt = C.c_uint32()
        call(self._L.smh_index_find, self._h, query._p, float(threshold), bool(containment), out, C.byref(cnt))
        return [int(out[i]) for i in range(cnt.value)]

    def most_common(self, leaf, downsample=False):
        if downsample:
            idx, q = self._meet_sketch(leaf)
            return idx.most_common(q)
        pos, cm = C.c_uint32(), C.c_uint64()
        call(self._L.smh_index_most_common, self._h, leaf._p, C.byref(pos), C.byref(cm))
        return pos.value, cm.value

    def gather(self, query, threshold_bp=0, scaled=None, max_rows=None, abund_stats=True, downsample=False):
        """Greedy decomposition of `query` against the resident sketches (smh_index_gather): GatherResult(rows, assigned).
        rows: one GatherRecord per round; assigned: uint32 numpy array, the round that consumed each query position (the
        hashes in ascending order) or UNASSIGNED.  threshold_common = ceil(threshold_bp / scaled); scaled defaults to the
        value the query's max_hash stands for.  The integers come from the device; the floats are derived here.  The
        device call leaves a query that lives in HBM where it is; f_unique_weighted, median_abund and std_abund of a query
        that tracks abundances need those on the host afterwards -- abund_stats=False leaves the three None instead.
        downsample=True: index and query meet at the smaller max_hash first; `scaled` then defaults to what that stands for,
        `assigned` runs over the positions of the cut query and the fractions are those of the cut query."""
        if downsample:
            idx, q = self._meet_sketch(query)
            return idx.gather(q, threshold_bp, scaled, max_rows, abund_stats)
        if scaled is None:
            mx = query.max_hash
            scaled = scaled_of_max_hash(mx) if mx else 1   # (a num query is refused by the call below)
        thr = int(math.ceil(threshold_bp / scaled))
        nq = len(query)
        cap = len(self) if max_rows is None else int(max_rows)
        rows = (SmhGatherRow * max(min(cap, len(self)), 1))()
        assigned = np.full(nq, UNASSIGNED, dtype=np.uint32)
        n_rows = C.c_uint32()
        call(self._L.smh_index_gather, self._h, query._p, thr, rows, cap, C.byref(n_rows),
             assigned.ctypes.data_as(C.POINTER(C.c_uint32)))
        return _gather_result(query, rows, n_rows.value, assigned, scaled, abund_stats)

    def gather_many(self, queries, threshold_bp=0, scaled=None, max_rows=None, abund_stats=True, downsample=False):
        """gather() of every query of a batch in one device call (smh_index_gather_many): a list of GatherResult, one per
        query in order, equal field for field to [self.gather(q, ...same arguments...) for q in queries].  The batch is
        looked up in the index's hash directory (built by the first such call, or by match(), and kept) and a round of every
        query shares one pair of launches.  downsample=True: the queries are grouped by the max_hash at which each meets
        the index; every group is one call."""
        queries = list(queries)
        if downsample:
            out = [None] * len(queries)
            for idx, members, cut in self._meet_groups(queries):
                for k, res in zip(members, idx.gather_many(cut, threshold_bp, scaled, max_rows, abund_stats)):
                    out[k] = res
            return out
        nqs = len(queries)
        scaleds, thrs = [], set()
        for q in queries:
            mx = q.max_hash
            sc = scaled if scaled is not None else scaled_of_max_hash(mx) if mx else 1
            scaleds.append(sc)
            thrs.add(int(math.ceil(threshold_bp / sc)))
        if len(thrs) > 1:   # (queries the call accepts share their max_hash; the others are refused by a call of their own)
            return [self.gather(q, threshold_bp, scaled, max_rows, abund_stats) for q in queries]
        thr = thrs.pop() if thrs else 0
        cap = len(self) if max_rows is None else int(max_rows)
        arr = (C.c_void_p * max(nqs, 1))(*[q._p for q in queries])
        row_off = np.zeros(nqs + 1, dtype=np.uint64)
        q_off = np.zeros(nqs + 1, dtype=np.uint64)
        assigned = np.empty(sum(len(q) for q in queries), dtype=np.uint32)   # (the call writes every entry)
        rows_p = C.POINTER(SmhGatherRow)()
        call(self._L.smh_index_gather_many, self._h, arr, nqs, thr, cap, row_off.ctypes.data_as(u64p), C.byref(rows_p),
             q_off.ctypes.data_as(u64p), assigned.ctypes.data_as(C.POINTER(C.c_uint32)))
        from .minhash import _free
        try:
            out = []
            for k, q in enumerate(queries):
                a, b = int(row_off[k]), int(row_off[k + 1])
                rows = [rows_p[r] for r in range(a, b)]
                out.append(_gather_result(q, rows, b - a, assigned[int(q_off[k]):int(q_off[k + 1])], scaleds[k], abund_stats))
        finally:
            _free(C.cast(rows_p, C.c_void_p))
        return out

    # --- the pairs over a threshold (additive ABI smh_index_search_*; the rules: include/sourmash_amd.h, smh_index_search_many)
    def _search_result(self, nqs, fn, *args):
        from .minhash import _free
        row_off = np.zeros(nqs + 1, dtype=np.uint64)
        rows_p = C.POINTER(SmhSearchRow)()
        call(fn, *args, row_off.ctypes.data_as(u64p), C.byref(rows_p))
        try:
            total = int(row_off[-1])
            rows = np.ctypeslib.as_array(C.cast(rows_p, C.POINTER(C.c_uint32)), shape=(total * 4,)).view(_SEARCH_ROW).copy() \
                if total else np.zeros(0, dtype=_SEARCH_ROW)
        finally:
            _free(C.cast(rows_p, C.c_void_p))
        first = self.nodes[0] if self.nodes else None
        return SearchResult(row_off, rows, first.ksize if first else None, first.molecule if first else None)

    @staticmethod
    def _threshold_common(threshold_bp, scaled):
        return int(math.ceil(threshold_bp / scaled))

    def _search_by_groups(self, queries, one_group):
        """the SearchResult of a batch whose queries meet the index at different max_hash: one_group(index, cut queries) per
        group, the rows put back in the batch's order"""
        parts = {}
        for idx, members, cut in self._meet_groups(queries):
            got = one_group(idx, cut)
            for j, k in enumerate(members):
                parts[k] = (got, got.rows_of(j))
        offsets = np.zeros(len(queries) + 1, dtype=np.uint64)
        rows = np.zeros(sum(sl.stop - sl.start for _, sl in parts.values()), dtype=_SEARCH_ROW)
        for k in range(len(queries)):
            got, sl = parts[k]
            a = int(offsets[k])
            offsets[k + 1] = a + sl.stop - sl.start
            for name in _SEARCH_ROW.names:
                rows[name][a:int(offsets[k + 1])] = getattr(got, name)[sl]
        first = self.nodes[0] if self.nodes else None
        return SearchResult(offsets, rows, first.ksize if first else None, first.molecule if first else None)

    def _batch_threshold_common(self, who, queries, threshold_bp, scaled):
        """ceil(threshold_bp / scaled) of a batch; scaled defaults to what the queries' max_hash stands for"""
        thrs = set()
        for q in queries:
            mx = q.max_hash
            thrs.add(self._threshold_common(threshold_bp, scaled if scaled is not None else scaled_of_max_hash(mx) if mx else 1))
        if len(thrs) > 1:   # (queries the call accepts share their max_hash)
            raise ValueError("%s: the queries differ in max_hash; give scaled, or downsample=True" % who)
        return thrs.pop() if thrs else 0

    def search_many(self, queries, threshold, metric="jaccard", threshold_bp=0, scaled=None, downsample=False):
        """The (query, node) pairs with metric > threshold and at least ceil(threshold_bp / scaled) hashes in common (one
        at least), from one device call (smh_index_search_many): a SearchResult.  metric: a key of SEARCH_METRICS.  scaled
        defaults to the value the queries' max_hash stands for.  Under "jaccard" / "containment_node" the nodes of query q are
        those of find(q, threshold) / find(q, threshold, containment=True).  downsample=True: the queries are grouped by the
        max_hash at which each meets the index; every group is one call, and the sizes are those of the cut sketches."""
        queries = list(queries)
        if downsample:
            return self._search_by_groups(queries, lambda idx, cut: idx.search_many(cut, threshold, metric, threshold_bp, scaled))
        nqs = len(queries)
        arr = (C.c_void_p * max(nqs, 1))(*[q._p for q in queries])
        return self._search_result(nqs, self._L.smh_index_search_many, self._h, arr, nqs, SEARCH_METRICS[metric], float(threshold),
                                   self._batch_threshold_common("search_many", queries, threshold_bp, scaled))

    def search_block_dev(self, hashes_dev, offsets, threshold, metric="jaccard", threshold_common=0, stream=None):
        """search_many of a CSR in device memory (smh_index_search_block_dev): query q is the hashes [offsets[q], offsets[q + 1])
        behind the device pointer hashes_dev, ascending strictly; offsets on the host.  A CSR has no `scaled`: the threshold on
        the common hashes is given as a count."""
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        nqs = len(offsets) - 1
        return self._search_result(nqs, lambda *a: self._L.smh_index_search_block_dev(*a, C.c_void_p(stream or 0)), self._h,
                                   C.c_void_p(hashes_dev), offsets.ctypes.data_as(u64p), nqs, SEARCH_METRICS[metric], float(threshold),
                                   int(threshold_common))

    def pairwise(self, threshold, metric="jaccard", threshold_bp=0, upper=True):
        """The index against itself (smh_index_search_self): the SearchResult of search_many of the index's own sketches
        without the rows node == query -- and, with upper=True, without the rows node < query.  The queries are read where
        they lie in HBM, so this works on an index downsample() returned (whose `nodes` are the uncut sketches): the node
        positions and the sizes are those of that index.  scaled is what the index's max_hash stands for."""
        lo, _ = self.max_hash_range
        thr = self._threshold_common(threshold_bp, scaled_of_max_hash(lo)) if lo else 0
        fn = self._L.smh_index_search_self
        return self._search_result(len(self), lambda h, m, t, c, *out: fn(h, m, t, c, bool(upper), *out), self._h, SEARCH_METRICS[metric],
                                   float(threshold), thr)

    # --- the best k of those pairs per query (additive ABI smh_index_nearest_*; the rules: include/sourmash_amd.h,
    # smh_index_nearest_many)
    def nearest(self, queries, k, metric="jaccard", threshold=0.0, threshold_bp=0, scaled=None, downsample=False):
        """Per query the k nearest nodes, best first, from one device call (smh_index_nearest_many): of the rows
        search_many(queries, threshold, metric, threshold_bp, scaled) reports for the query, the first k by the metric's value
        descending, then node ascending -- a SearchResult whose rows are in that order.  A node that shares no hash with the
        query is never a neighbour, so a query may get fewer than k rows.  1 <= k <= matrix.nearest_geometry()[0].
        downsample=True groups the queries as search_many does."""
        queries = list(queries)
        if downsample:
            return self._search_by_groups(queries, lambda idx, cut: idx.nearest(cut, k, metric, threshold, threshold_bp, scaled))
        nqs = len(queries)
        arr = (C.c_void_p * max(nqs, 1))(*[q._p for q in queries])
        return self._search_result(nqs, self._L.smh_index_nearest_many, self._h, arr, nqs, int(k), SEARCH_METRICS[metric], float(threshold),
                                   self._batch_threshold_common("nearest", queries, threshold_bp, scaled))

    def nearest_block_dev(self, hashes_dev, offsets, k, metric="jaccard", threshold=0.0, threshold_common=0, stream=None):
        """nearest of a CSR in device memory (smh_index_nearest_block_dev), with the contract of search_block_dev"""
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        nqs = len(offsets) - 1
        return self._search_result(nqs, lambda *a: self._L.smh_index_nearest_block_dev(*a, C.c_void_p(stream or 0)), self._h,
                                   C.c_void_p(hashes_dev), offsets.ctypes.data_as(u64p), nqs, int(k), SEARCH_METRICS[metric], float(threshold),
                                   int(threshold_common))

    def knn(self, k, metric="jaccard", threshold=0.0, threshold_bp=0):
        """The k-nearest-neighbour graph of the index (smh_index_nearest_self): nearest of the index's own sketches, read where
        they lie in HBM, without the rows node == query.  Works on an index downsample() returned, as pairwise does; scaled is
        what the index's max_hash stands for."""
        lo, _ = self.max_hash_range
        thr = self._threshold_common(threshold_bp, scaled_of_max_hash(lo)) if lo else 0
        return self._search_result(len(self), self._L.smh_index_nearest_self, self._h, int(k), SEARCH_METRICS[metric], float(threshold), thr)

    # --- clustering (additive ABI smh_index_cluster; the rules: include/sourmash_amd.h, smh_index_cluster)
    def cluster(self, threshold, metric="jaccard", linkage="components", scores=None, threshold_bp=0, scaled=None, ani=False):
        """The clusters of the index's nodes, made on the device (smh_index_cluster): a Clustering.  Two nodes are adjacent iff
        pairwise(threshold, metric, threshold_bp) reports the pair; metric: "jaccard" or "max_containment".  linkage
        "components": single linkage, the connected components; "greedy": the best-scored node first, everything adjacent to a
        representative joins the closest one, and nothing chains.  scores (n integers below 2^32; default: the sketch sizes)
        rank the nodes, ties go to the lower node.  ani=True reads `threshold` as an average nucleotide identity and clusters
        at max_containment > threshold ** ksize: DNA sketches and metric="max_containment" only.  scaled defaults to what the
        index's max_hash stands for.  Works on an index downsample() returned: the nodes are the cut ones."""
        if ani:
            first = self.nodes[0] if self.nodes else None
            if metric != "max_containment":
                raise ValueError("ani=True takes metric='max_containment', not %r" % (metric,))
            if first is None or first.molecule != "DNA" or not first.ksize:
                raise ValueError("ani is defined for DNA sketches only (this index: %s)" % (first.molecule if first else "no nodes"))
            threshold = float(threshold) ** first.ksize
        if metric not in ("jaccard", "max_containment"):
            raise ValueError("cluster takes the symmetric metrics 'jaccard' and 'max_containment', not %r" % (metric,))
        n = len(self)
        lo, _ = self.max_hash_range
        thr = self._threshold_common(threshold_bp, scaled if scaled is not None else scaled_of_max_hash(lo)) if lo else 0
        greedy = CLUSTER_LINKAGES[linkage] == 1
        sc = None
        if scores is not None:
            sc = np.ascontiguousarray(scores, dtype=np.uint32)
            if sc.shape != (n,):
                raise ValueError("scores: one per node")
        cl, rep = np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint32)   # (never a NULL pointer)
        common = np.zeros(max(n, 1), dtype=np.uint32) if greedy else None
        k = C.c_uint32()
        call(self._L.smh_index_cluster, self._h, SEARCH_METRICS[metric], float(threshold), thr, CLUSTER_LINKAGES[linkage],
             sc.ctypes.data_as(u32p) if sc is not None else None, cl.ctypes.data_as(u32p), rep.ctypes.data_as(u32p),
             common.ctypes.data_as(u32p) if greedy else None, C.byref(k))
        return Clustering(cl[:n], rep[:n], k.value, common[:n] if greedy else None, self.sizes() if greedy else None, metric)

    def sizes(self):
        """|S_v| of every node as the index holds it (uint32; smh_index_sizes): for an index downsample() returned, the sizes of
        the cut sketches"""
        n = len(self)
        out = np.zeros(max(n, 1), dtype=np.uint32)
        call(self._L.smh_index_sizes, self._h, out.ctypes.data_as(u32p))
        return out[:n]

    # --- collapsing by groups and the read-back (additive ABI smh_index_collapse, smh_index_read; the rules:
    # include/sourmash_amd.h, "Collapsing an index by groups")
    def collapse(self, groups, n_groups=None, min_count=1, min_fraction=0.0, abund="flat"):
        """One sketch per group of nodes, made on the device (smh_index_collapse): a ResidentIndex of n_groups nodes.  Sketch g
        holds the hashes that at least max(1, min_count, ceil(min_fraction * members)) members of group g hold: the defaults
        give the union (`sig merge`), min_fraction=1.0 the core (`sig intersect`).  groups: one int per node, None or -1 for a
        node that takes no part -- or a Clustering, whose clusters are the groups: idx.collapse(idx.cluster(0.9,
        metric="max_containment")) is the pangenome sketch of every cluster.  n_groups defaults to the largest group + 1.
        abund: a key of COLLAPSE_ABUNDS -- "flat" none, "sum" the members' abundances added up, "count" the number of members
        that hold the hash.  The result carries no taxonomy and its `nodes` are its own sketches, read back when first asked."""
        if isinstance(groups, Clustering):
            if n_groups is None:
                n_groups = groups.n_clusters
            g = np.ascontiguousarray(groups.cluster, dtype=np.uint32)
        else:
            wide = np.array([-1 if x is None else int(x) for x in groups], dtype=np.int64)
            if wide.size and (wide.min() < -1 or wide.max() >= COLLAPSE_DROP):
                raise ValueError("groups: ints in [0, 2^32 - 1), None or -1")
            if n_groups is None:
                n_groups = int(wide.max()) + 1 if wide.size else 0
            g = np.where(wide < 0, COLLAPSE_DROP, wide).astype(np.uint32)
        if g.shape != (len(self),):
            raise ValueError("groups: one per node")
        if g.size == 0:
            g = np.zeros(1, dtype=np.uint32)   # (never a NULL pointer)
        track = COLLAPSE_ABUNDS[abund] != 0
        child = ResidentIndex((), _handle=call(self._L.smh_index_collapse, self._h, g.ctypes.data_as(u32p), int(n_groups), int(min_count),
                                               float(min_fraction), COLLAPSE_ABUNDS[abund]))
        first = self.nodes[0] if len(self.nodes) else None
        lo, _ = self.max_hash_range
        child._template = (0, first.ksize, first.molecule, first.seed, lo, track) if first is not None else \
            (0, 21, "DNA", 42, (1 << 64) - 1, track)
        child.nodes = _OwnSketches(child)
        return child

    def read(self):
        """The index as it is held (smh_index_read): (offsets, hashes, abunds) -- uint64 offsets of len(self) + 1 entries from
        0, the uint64 hashes of node v at [offsets[v], offsets[v + 1]), and their uint32 abundances, or None for an index
        without abundances.  For an index downsample() or collapse() returned these are the cut / collapsed sketches."""
        n = len(self)
        off = np.zeros(n + 1, dtype=np.uint64)
        call(self._L.smh_index_read, self._h, off.ctypes.data_as(u64p), None, None)
        total = int(off[-1])
        hashes = np.zeros(max(total, 1), dtype=np.uint64)
        abunds = np.zeros(max(total, 1), dtype=np.uint32) if self.has_abundances else None
        call(self._L.smh_index_read, self._h, None, hashes.ctypes.data_as(u64p), abunds.ctypes.data_as(u32p) if abunds is not None else None)
        return off, hashes[:total], abunds[:total] if abunds is not None else None

    def sketches(self):
        """The nodes as the index holds them, a list of KmerMinHash filled through smh_index_read: a node's own num, ksize,
        molecule and seed, the max_hash of the index (for downsample()'s result: the cut one), abundances when the index has
        them.  For collapse()'s result the parameters are those the collapsed index took from its parent."""
        from .minhash import KmerMinHash
        off, hashes, abunds = self.read()
        lo, hi = self.max_hash_range
        template = getattr(self, "_template", None)
        per_node = getattr(self, "_node_templates", None)   # concat()'s result: the parameters its parts' nodes had
        out = []
        for v in range(len(self)):
            if per_node is not None:
                num, ksize, molecule, seed, mx, _ = per_node[v]
                track = abunds is not None
            elif template is not None:
                num, ksize, molecule, seed, mx, track = template
            else:
                node = self.nodes[v]
                num, ksize, molecule, seed, track = node.num, node.ksize, node.molecule, node.seed, abunds is not None
                mx = lo if lo == hi else node.max_hash
            mh = KmerMinHash(num, ksize, False, seed, mx, track, alphabet=None if molecule == "DNA" else molecule)
            a, b = int(off[v]), int(off[v + 1])
            if b > a and abunds is not None:
                h64, a64 = np.ascontiguousarray(hashes[a:b]), abunds[a:b].astype(np.uint64)
                call(self._L.smh_add_many_with_abund, mh._p, h64.ctypes.data_as(u64p), a64.ctypes.data_as(u64p), b - a)
            elif b > a:
                mh.add_many(hashes[a:b])
            out.append(mh)
        return out

    # --- signature JSON written on the device (additive ABI smh_index_sigtext, smh_sigtext_*, smh_index_md5; the rules:
    # include/sourmash_amd.h, "Signature JSON written on the device")
    def sigtext(self, names=None, filenames=None, doc_starts=None):
        """The index as `.sig` text in HBM: a signature.SigText.  names / filenames: one str or None per node
        (None: a JSON null); they default to those of `self.signatures` where from_signatures left them, else to null.
        doc_starts: n_docs + 1 ascending node numbers from 0 to len(self), document d = the nodes [doc_starts[d],
        doc_starts[d + 1]); None: one document."""
        from .signature import SigText
        n = len(self)
        entries = getattr(self, "signatures", None)
        if names is None and entries is not None:
            names = [e.name for e in entries]
        if filenames is None and entries is not None:
            filenames = [e.filename for e in entries]

        def strings(v, what):
            if v is None:
                return None
            v = list(v)
            if len(v) != n:
                raise ValueError("%s: one per node" % what)
            return (C.c_char_p * max(n, 1))(*[None if s is None else s.encode("utf-8") for s in v])
        ds, n_docs = None, 0
        if doc_starts is not None:
            wide = np.asarray(doc_starts, dtype=np.int64).reshape(-1)
            if wide.size < 1 or wide.min() < 0 or wide.max() > 0xFFFFFFFF:
                raise ValueError("doc_starts: one more entry than documents, ints in [0, 2^32)")
            ds = np.ascontiguousarray(wide, dtype=np.uint32)
            n_docs = ds.size - 1
        return SigText(call(self._L.smh_index_sigtext, self._h, strings(names, "names"), strings(filenames, "filenames"),
                            ds.ctypes.data_as(u32p) if ds is not None else None, n_docs))

    def save_signatures(self, path=None, names=None, filenames=None, doc_starts=None, device=False):
        """The byte string signature.save_signatures gives for sketches() -- each in a default Signature with its name and
        filename, the documents of doc_starts one after another -- formatted on the device (sigtext()).  Returns bytes; with
        device=True (a CUDA uint8 tensor of its own, doc_offsets).  path: the text is also written to that file."""
        t = self.sigtext(names, filenames, doc_starts)
        if device and path is None:
            return t.tensor(), t.doc_offsets
        data = t.read()
        if path is not None:
            with open(path, "wb") as fh:
                fh.write(data)
        return (t.tensor(), t.doc_offsets) if device else data

    def md5sums(self):
        """every node's md5sum as sourmash names it, 32 hex digits: of str(ksize) and the decimal hashes (smh_index_md5)"""
        n = len(self)
        out = np.zeros(max(n, 1) * 16, dtype=np.uint8)
        call(self._L.smh_index_md5, self._h, out.ctypes.data_as(C.c_void_p))
        return [out[16 * v:16 * v + 16].tobytes().hex() for v in range(n)]

    # --- building from records, concatenation (additive ABI smh_index_from_*, smh_index_concat; the rules: include/sourmash_amd.h,
    # "Building an index from records")
    @classmethod
    def from_records(cls, records, like, groups=None, n_groups=None, amino=False, stream=None):
        """An index built from the records of a batch without leaving the device (smh_index_from_*): node g holds what the
        records of group g leave in a fresh sketch of `like`'s parameters (force=True semantics: windows with a byte outside
        ACGT are skipped).  records: a fastx.Records, a list of bytes, or (dev_ptr, total_len, offsets), as match() takes
        them.  like: a scaled KmerMinHash; only its parameters are read.  groups: one int per record (None: record r is node
        r); n_groups defaults to max(groups) + 1, or to the number of records.  amino=True: the records are amino-acid
        sequences (`like` is a protein, dayhoff or hp sketch).  The result's `nodes` are its own sketches, read back when
        first asked."""
        from .fastx import Records
        L = lib()
        if isinstance(records, Records):
            n = len(records)
        elif isinstance(records, tuple):
            ptr, total, offsets = records
            offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
            n = len(offsets) - 1
        else:
            seqs = [bytes(s) for s in records]
            n = len(seqs)
        g = None
        if groups is not None:
            wide = np.asarray(groups, dtype=np.int64)
            if wide.shape != (n,):
                raise ValueError("groups: one per record")
            if wide.size and (wide.min() < 0 or wide.max() > 0xFFFFFFFF):
                raise ValueError("groups: ints in [0, 2^32)")
            if n_groups is None:
                n_groups = int(wide.max()) + 1 if wide.size else 0
            g = np.ascontiguousarray(wide, dtype=np.uint32)
            if g.size == 0:
                g = np.zeros(1, dtype=np.uint32)   # (never a NULL pointer: NULL means one node per record)
        elif n_groups is None:
            n_groups = n
        gp = g.ctypes.data_as(u32p) if g is not None else None
        kind = 1 if amino else 0
        if isinstance(records, Records):
            h = call(L.smh_index_from_records, like._p, kind, records._p, gp, int(n_groups))
        elif isinstance(records, tuple):
            h = call(L.smh_index_from_sequences_dev, like._p, kind, C.c_void_p(ptr), int(total), offsets.ctypes.data_as(u64p), gp, n,
                     int(n_groups), C.c_void_p(stream or 0))
        else:
            offsets = np.zeros(n + 1, dtype=np.uint64)
            np.cumsum(np.array([len(s) for s in seqs], dtype=np.uint64), out=offsets[1:])
            h = call(L.smh_index_from_sequences, like._p, kind, b"".join(seqs), offsets.ctypes.data_as(u64p), gp, n, int(n_groups))
        idx = cls((), _handle=h)
        idx._template = (0, like.ksize, like.molecule, like.seed, like.max_hash, bool(like.track_abundance))
        idx.nodes = _OwnSketches(idx)
        return idx

    # --- from signature JSON read on the device (additive ABI smh_signatures_*, smh_signatures_index*; the rules:
    # include/sourmash_amd.h, "Signature JSON on the device")
    @classmethod
    def from_signatures(cls, source, ksize=0, moltype=None, ids=None, stream=None):
        """An index of the sketches of signature JSON whose numbers were read on the device: the hashes go
        from the text's values to the index device to device.  source: a signature.SignatureScan; bytes of one document; a
        path or a list of paths (plain files and single-stream gzip are read on the host, concatenated and uploaded once; a
        blocked-gzip file is inflated on the device; a path or bytes that begin PK\\3\\4 are a zip collection and go to from_zip).
        ids: the scan's entries to take, any order, repeats allowed; None: the
        entries load_signatures' filter keeps for ksize (0: any) and moltype (None: any).  The index answers every call as
        ResidentIndex(load_signatures_buffer(...)) does; one refusal of its own (code 3): hashes that are not strictly
        ascending.  `signatures` holds the chosen entries; `nodes` are the index's own sketches, read back when first asked."""
        from .signature import SignatureScan, read_signature_text
        from .archive import is_zip
        L = lib()
        if ids is None and not isinstance(source, (SignatureScan, list, tuple)) and is_zip(source):
            return cls.from_zip(source, ksize=ksize, moltype=moltype, stream=stream)   # a zip collection (bytes or a path)
        if isinstance(source, SignatureScan):
            scan = source
        elif isinstance(source, (bytes, bytearray, memoryview)):
            scan = SignatureScan.parse(source, stream=stream)
        else:
            data, offs = read_signature_text(source)
            scan = SignatureScan.parse(data, offs, stream=stream)
        entries = scan.entries
        if ids is None:                                   # the filter exists once, in the library: its ids are the choice
            v = np.zeros(max(len(entries), 1), dtype=np.uint32)
            kept = call(L.smh_signatures_filter, scan._p, int(ksize), moltype.encode() if moltype else None, v.ctypes.data_as(u32p))
            v = v[:kept]
        else:
            wide = np.asarray(ids, dtype=np.int64).reshape(-1)
            if wide.size and (wide.min() < 0 or wide.max() > 0xFFFFFFFF):
                raise ValueError("from_signatures: ids are ints in [0, 2^32)")
            v = np.ascontiguousarray(wide, dtype=np.uint32)
        chosen = [int(i) for i in v]
        h = call(L.smh_signatures_index, scan._p, (v if v.size else np.zeros(1, np.uint32)).ctypes.data_as(u32p), int(v.size))
        idx = cls((), _handle=h)
        idx.signatures = [entries[i] for i in chosen]
        track = idx.has_abundances
        idx._node_templates = [(e.num, e.ksize, e.molecule, e.seed, e.max_hash, track) for e in idx.signatures]
        idx.nodes = _OwnSketches(idx)
        return idx

    @classmethod
    def from_zip(cls, source, ksize=0, moltype=None, md5=None, device_member_limit=None, stream=None):
        """An index of the sketches of a zip collection: the compressed file is uploaded once, the chosen
        members are inflated on the device (archive.ZipCollection.text), read there (SignatureScan.parse) and gathered device
        to device (from_signatures).  source: a path, the archive's bytes, or an archive.ZipCollection.  The members are
        chosen by the manifest where there is one (ZipCollection.select); the sketches by the library's own filter for ksize
        (0: any) and moltype (None: any), and by md5 (a string or a collection of them) against each sketch's `md5sum`.
        device_member_limit: members whose text is larger are inflated on the host (None: the default).  `signatures` holds
        the chosen entries, as from_signatures leaves them."""
        from .archive import ZipCollection
        from .signature import SignatureScan
        L = lib()
        zc = source if isinstance(source, ZipCollection) else ZipCollection(source)
        members = zc.select(ksize=ksize, moltype=moltype, md5=md5)
        text, offs = zc.text(members, device_member_limit=device_member_limit, stream=stream)
        scan = SignatureScan.parse(text, offs, stream=stream)
        v = np.zeros(max(len(scan), 1), dtype=np.uint32)
        kept = call(L.smh_signatures_filter, scan._p, int(ksize), moltype.encode() if moltype else None, v.ctypes.data_as(u32p))
        chosen = [int(i) for i in v[:kept]]
        if md5 is not None:
            md5s = {md5} if isinstance(md5, str) else set(md5)
            entries = scan.entries
            chosen = [i for i in chosen if entries[i].md5sum in md5s]
        return cls.from_signatures(scan, ids=chosen, stream=stream)

    @classmethod
    def concat(cls, parts):
        """A new index whose nodes are those of parts[0], then parts[1], ... (smh_index_concat): device-to-device copies, no
        rebuild through the host.  Parts may be any resident indexes; abundances are kept when every part has them; no
        taxonomy is carried over.  The result owns its memory, and its `nodes` are its own sketches, read back when first
        asked."""
        parts = list(parts)
        L = lib()
        arr = (C.c_void_p * max(len(parts), 1))(*[p._h for p in parts])
        idx = cls((), _handle=call(L.smh_index_concat, arr, len(parts)))
        idx._node_templates = _PartParams(parts)
        idx.nodes = _OwnSketches(idx)
        return idx

    # --- filtering the nodes, taking a subset of them (additive ABI smh_index_filter, smh_index_select; the rules:
    # include/sourmash_amd.h, "Filtering an index")
    def filter(self, operand=None, mode=None, abund="own", min_abund=0, max_abund=None, min_owners=0, max_owners=None, downsample=False):
        """This index with every node cut down to the hashes that pass a rule, made on the device (smh_index_filter): a
        ResidentIndex of the same nodes in the same order, with this index's taxonomy.  A hash of a node is kept when all of
        these hold, each judged on THIS index: mode "keep" -- it is in `operand`, "drop" -- it is not (None: no operand);
        min_abund <= the node's abundance of it <= max_abund; min_owners <= the nodes of this index that hold it <= max_owners
        (max_owners=1: every node's private hashes; min_owners=2: the shared ones).  abund: a key of FILTER_ABUNDS -- "own" the
        kept hashes keep their abundances, "flat" none, "operand" the operand's abundance of the hash (mode "keep").
        downsample=True: operand and index meet at the coarser max_hash of the two.  The result's `nodes` are its own
        sketches, read back when first asked."""
        if mode not in FILTER_MODES or (mode is None) != (operand is None):
            raise ValueError("mode: 'keep' or 'drop' with an operand, None without")
        if downsample and operand is not None:
            idx, q = self._meet_sketch(operand)
            return idx.filter(q, mode, abund, min_abund, max_abund, min_owners, max_owners)
        rule = SmhFilter(FILTER_MODES[mode], FILTER_ABUNDS[abund], int(min_abund), FILTER_NO_MAX if max_abund is None else int(max_abund),
                         int(min_owners), FILTER_NO_MAX if max_owners is None else int(max_owners))
        child = ResidentIndex((), _handle=call(self._L.smh_index_filter, self._h, operand._p if operand is not None else None, C.byref(rule)))
        child._node_templates = _PartParams([self])
        child.nodes = _OwnSketches(child)
        return child

    def subtract(self, query, downsample=False):
        """every node without the hashes of `query` (`sig subtract`)"""
        return self.filter(query, "drop", downsample=downsample)

    def intersect(self, query, downsample=False):
        """every node restricted to the hashes of `query` (`sig intersect` against a mask)"""
        return self.filter(query, "keep", downsample=downsample)

    def inflate(self, query, downsample=False):
        """every node restricted to the hashes of `query`, with query's abundances (`sig inflate`)"""
        return self.filter(query, "keep", abund="operand", downsample=downsample)

    def flatten(self):
        """the same nodes without abundances (`sig flatten`)"""
        return self.filter(abund="flat")

    def select(self, ids):
        """A new index whose node j is node ids[j] of this one, whole, copied on the device (smh_index_select): any order,
        repeats allowed; or a boolean mask of len(self) entries (the nodes where it is True, in order).  Works on every index;
        abundances and the taxonomy go with the nodes.  The result's `nodes` are its own sketches, read back when first
        asked."""
        arr = np.asarray(ids)
        if arr.dtype == np.bool_:
            if arr.shape != (len(self),):
                raise ValueError("select: a boolean mask has one entry per node")
            arr = np.flatnonzero(arr)
        wide = arr.astype(np.int64).reshape(-1)
        if wide.size and (wide.min() < 0 or wide.max() > 0xFFFFFFFF):
            raise ValueError("select: ids are ints in [0, 2^32)")
        v = np.ascontiguousarray(wide, dtype=np.uint32)
        child = ResidentIndex((), _handle=call(self._L.smh_index_select, self._h, (v if v.size else np.zeros(1, np.uint32)).ctypes.data_as(u32p),
                                               int(v.size)))
        child._node_templates = _PickedParams(_PartParams([self]), v)
        child.nodes = _OwnSketches(child)
        return child

    def match(self, records, hits=False, stream=None):
        """Every record of a batch against the index (smh_index_match_*; the rules: include/sourmash_amd.h, "Matching
        records"): MatchResult of numpy arrays, one entry per record.  records: a fastx.Records, a list of bytes, or
        (dev_ptr, total_len, offsets) for a batch in device memory.  hits=True also returns the CSR of every record's
        distinct hit hashes, ascending.  best is NO_MATCH for a record without a hit.  There is no downsample argument:
        raw records have no resolution of their own, they are sampled at the index's max_hash."""
        from .fastx import Records
        from .minhash import _free
        hp, nh = u64p(), C.c_uint64()

        def run(n, fn, *front):
            rows = np.zeros(n, dtype=_MATCH_ROW)
            off = np.zeros(n + 1, dtype=np.uint64) if hits else None
            tail = (off.ctypes.data_as(u64p), C.byref(hp), C.byref(nh)) if hits else (None, None, None)
            call(fn, self._h, *front, rows.ctypes.data_as(C.c_void_p), *tail)
            return rows, off

        if isinstance(records, Records):
            rows, off = run(len(records), self._L.smh_index_match_records, records._p)
        elif isinstance(records, tuple):
            ptr, total, offsets = records
            offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
            rows, off = run(len(offsets) - 1, lambda h, *a: self._L.smh_index_match_sequences_dev(h, *a, C.c_void_p(stream or 0)),
                            C.c_void_p(ptr), int(total), offsets.ctypes.data_as(u64p), len(offsets) - 1)
        else:
            seqs = [bytes(s) for s in records]
            offsets = np.zeros(len(seqs) + 1, dtype=np.uint64)
            np.cumsum(np.array([len(s) for s in seqs], dtype=np.uint64), out=offsets[1:])
            rows, off = run(len(seqs), self._L.smh_index_match_sequences, b"".join(seqs), offsets.ctypes.data_as(u64p), len(seqs))
        hashes = None
        if hits:
            hashes = np.ctypeslib.as_array(hp, shape=(nh.value,)).copy() if nh.value else np.zeros(0, np.uint64)
            _free(C.cast(hp, C.c_void_p))
        return MatchResult(*[rows[name] for name in _MATCH_ROW.names], off, hashes)   # views of the rows: no copy

    # --- taxonomic LCA (additive ABI smh_index_*taxonomy, smh_index_lca_*; the rules: include/sourmash_amd.h, "Taxonomic LCA")
    def set_taxonomy(self, parent, node_taxon):
        """parent[t] of every taxon (taxon 0 is the root, parent[t] < t) and the taxon of every node (NO_TAXON: none).  Replaces
        an earlier taxonomy; the cut indexes downsample() cached are given back (a child takes its taxonomy when it is made)."""
        parent = np.ascontiguousarray(parent, dtype=np.uint32)
        node_taxon = np.ascontiguousarray(node_taxon, dtype=np.uint32)
        call(self._L.smh_index_set_taxonomy, self._h, parent.ctypes.data_as(u32p), len(parent), node_taxon.ctypes.data_as(u32p),
             len(node_taxon))
        self._children.clear()

    @property
    def has_taxonomy(self):
        return bool(self._L.smh_index_has_taxonomy(self._h))

    def lca_counts(self, queries, hash_taxon=False, downsample=False):
        """Per query (taxa, counts): the taxa of its assigned hashes ascending (uint32) and how many hashes each got (uint64),
        from one device call (smh_index_lca_many).  hash_taxon=True: per query (taxa, counts, per_hash), per_hash the taxon of
        every hash of the query in ascending hash order or NO_TAXON.  downsample=True: the queries are grouped by the max_hash
        at which each meets the index, every group is one call; per_hash then runs over the hashes of the cut query."""
        queries = list(queries)
        if downsample:
            out = [None] * len(queries)
            for idx, members, cut in self._meet_groups(queries):
                for k, res in zip(members, idx.lca_counts(cut, hash_taxon)):
                    out[k] = res
            return out
        nqs = len(queries)
        arr = (C.c_void_p * max(nqs, 1))(*[q._p for q in queries])
        c_off = np.zeros(nqs + 1, dtype=np.uint64)
        q_off = np.zeros(nqs + 1, dtype=np.uint64)
        per = np.empty(sum(len(q) for q in queries), dtype=np.uint32) if hash_taxon else None
        tp, cp = u32p(), u64p()
        call(self._L.smh_index_lca_many, self._h, arr, nqs, c_off.ctypes.data_as(u64p), C.byref(tp), C.byref(cp),
             q_off.ctypes.data_as(u64p), per.ctypes.data_as(u32p) if hash_taxon else None)
        return self._lca_split(tp, cp, c_off, q_off, per)

    def lca_counts_block_dev(self, hashes_dev, offsets, hash_taxon=False, stream=None):
        """lca_counts of a CSR in device memory (smh_index_lca_block_dev): query q is the hashes [offsets[q], offsets[q + 1])
        behind the device pointer hashes_dev, ascending strictly; offsets on the host."""
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        nqs = len(offsets) - 1
        c_off = np.zeros(nqs + 1, dtype=np.uint64)
        per = np.empty(int(offsets[-1] - offsets[0]), dtype=np.uint32) if hash_taxon else None
        tp, cp = u32p(), u64p()
        call(self._L.smh_index_lca_block_dev, self._h, C.c_void_p(hashes_dev), offsets.ctypes.data_as(u64p), nqs,
             c_off.ctypes.data_as(u64p), C.byref(tp), C.byref(cp), per.ctypes.data_as(u32p) if hash_taxon else None,
             C.c_void_p(stream or 0))
        return self._lca_split(tp, cp, c_off, offsets - offsets[0], per)

    @staticmethod
    def _lca_split(tp, cp, c_off, q_off, per):
        from .minhash import _free
        total = int(c_off[-1])
        try:
            taxa = np.ctypeslib.as_array(tp, shape=(total,)).copy() if total else np.zeros(0, np.uint32)
            counts = np.ctypeslib.as_array(cp, shape=(total,)).copy() if total else np.zeros(0, np.uint64)
        finally:
            _free(C.cast(tp, C.c_void_p))
            _free(C.cast(cp, C.c_void_p))
        out = []
        for k in range(len(c_off) - 1):
            a, b = int(c_off[k]), int(c_off[k + 1])
            one = (taxa[a:b], counts[a:b])
            out.append(one + (per[int(q_off[k]):int(q_off[k + 1])],) if per is not None else one)
        return out

    def lca_classify_records(self, records, stream=None):
        """Every record of a batch classified (smh_index_lca_*): LcaRecords of numpy arrays, one entry per record.  records: the
        three forms match() takes.  taxon is NO_TAXON and status LCA_NONE for a record without an assigned hit; status is
        LCA_FOUND or LCA_DISAGREE otherwise."""
        from .fastx import Records

        def run(n, fn, *front):
            rows = np.zeros(n, dtype=_LCA_ROW)
            call(fn, self._h, *front, rows.ctypes.data_as(C.c_void_p))
            return rows

        if isinstance(records, Records):
            rows = run(len(records), self._L.smh_index_lca_records, records._p)
        elif isinstance(records, tuple):
            ptr, total, offsets = records
            offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
            rows = run(len(offsets) - 1, lambda h, *a: self._L.smh_index_lca_sequences_dev(h, *a, C.c_void_p(stream or 0)),
                       C.c_void_p(ptr), int(total), offsets.ctypes.data_as(u64p), len(offsets) - 1)
        else:
            seqs = [bytes(s) for s in records]
            offsets = np.zeros(len(seqs) + 1, dtype=np.uint64)
            np.cumsum(np.array([len(s) for s in seqs], dtype=np.uint64), out=offsets[1:])
            rows = run(len(seqs), self._L.smh_index_lca_sequences, b"".join(seqs), offsets.ctypes.data_as(u64p), len(seqs))
        return LcaRecords(*[rows[name] for name in _LCA_ROW.names])   # views of the rows: no copy

    @property
    def has_abundances(self):
        """every node tracked abundances when the index was built: the angular calls below can be served"""
        return bool(self._L.smh_index_has_abundances(self._h))

    def norms2(self):
        """norm2 of every node (the sum of its squared abundances), uint64"""
        out = np.zeros(len(self), dtype=np.uint64)
        call(self._L.smh_index_norms2, self._h, out.ctypes.data_as(u64p))
        return out

    def angular(self, query, downsample=False):
        """`query` against every node (smh_index_angular_query): AngularResult(dot, cosine, angular), numpy arrays of
        len(self) entries.  A query that lives in HBM stays there."""
        if downsample:
            idx, q = self._meet_sketch(query)
            return idx.angular(q)
        n = len(self)
        dot, cos, ang = np.zeros(n, np.uint64), np.zeros(n, np.float64), np.zeros(n, np.float64)
        f64p = C.POINTER(C.c_double)
        call(self._L.smh_index_angular_query, self._h, query._p, dot.ctypes.data_as(u64p), None, cos.ctypes.data_as(f64p),
             ang.ctypes.data_as(f64p))
        return AngularResult(dot, cos, ang)

    def angular_matrix(self, other=None, want=("angular",), downsample=False):
        """len(self) x len(other) matrix (other=None: the index against itself, symmetric) -> dict name -> array;
        names: dot, cosine, angular (smh_index_angular)."""
        other = self if other is None else other
        if downsample:
            a, b = self._meet_index(other)
            return a.angular_matrix(b, want)
        kinds = {"dot": np.uint64, "cosine": np.float64, "angular": np.float64}
        out = {k: np.zeros((len(self), len(other)), dtype=kinds[k]) for k in want}

        def p(name):
            if name not in out:
                return None
            return out[name].ctypes.data_as(C.POINTER(C.c_double) if out[name].dtype == np.float64 else u64p)

        call(self._L.smh_index_angular, self._h, other._h, p("dot"), p("cosine"), p("angular"))
        return out

    def compare(self, other, want=("jaccard",), downsample=False):
        if downsample:
            a, b = self._meet_index(other)
            return a.compare(b, want)
        n, m = len(self), len(other)
        kinds = {"jaccard": np.float64, "common": np.uint64, "size": np.uint64, "count_common": np.uint64,
                 "containment": np.float64}
        out = {k: np.zeros((n, m), dtype=kinds[k]) for k in want}

        def p(name):
            if name not in out:
                return None
            return out[name].ctypes.data_as(C.POINTER(C.c_double) if out[name].dtype == np.float64 else u64p)

        call(self._L.smh_index_compare, self._h, other._h, p("jaccard"), p("common"), p("size"), p("count_common"),
             p("containment"))
        return out


class LinearIndex:
    """reference src/index/linear.rs: leaves + find(search_fn, query, threshold).  The leaves are
    mirrored in HBM on the first find after an insert."""

    def __init__(self):
        self.leaves = []
        self._resident = None

    def insert(self, mh):
        self.leaves.append(mh)
        self._resident = None

    def find(self, search_fn, query, threshold):
        if search_fn in (search_minhashes, search_minhashes_containment):
            if self._resident is None:
                self._resident = ResidentIndex(self.leaves)
            hits = self._resident.find(query, threshold, containment=search_fn is search_minhashes_containment)
        else:
            hits = search_fn(self.leaves, query, threshold)
        return [self.leaves[i] for i in hits]


def most_common(leaf, candidates):
    """(position, count_common) of the candidate sharing the most hashes with `leaf`."""
    n = len(candidates)
    arr = (C.c_void_p * max(n, 1))(*[m._p for m in candidates])
    pos, cm = C.c_uint32(), C.c_uint64()
    call(lib().smh_most_common, leaf._p, arr, n, C.byref(pos), C.byref(cm))
    return pos.value, cm.value


def scaffold_pairs(datasets):
    """The leaf-pairing pass of the reference's scaffold (src/index/sbt.rs:356-373): pop the last
    leaf, pair it with the remaining leaf sharing the most hashes, repeat.  Returns the pairs."""
    datasets = list(datasets)
    pairs = []
    while datasets:
        nxt = datasets.pop()
        if not datasets:
            pairs.append((nxt, None))
            break
        pos, _ = most_common(nxt, datasets)
        pairs.append((nxt, datasets.pop(pos)))
    return pairs
