"""Clustering a resident index restated in plain sequential Python (the rules of include/sourmash_amd.h, smh_index_cluster;
DESIGN.md 3.17).

No product import: this is what the device kernels are compared against, entry for entry.  The adjacency is the rule of the
thresholded search (search_many_restatement.reported) on every pair of sketches.

    sketches          list of iterables of hashes (S_0 .. S_{n-1})
    metric            JACCARD or MAX_CONTAINMENT (the symmetric ones)
    threshold         a float; the comparison is strict
    threshold_common  0 is read as 1
    linkage           COMPONENTS or GREEDY
    scores            n integers, or None for |S_v|

A graph is a list adj of n dicts: adj[v][u] = (value, common) for every neighbour u of v, both directions present."""
import search_many_restatement as SR

JACCARD, MAX_CONTAINMENT = SR.JACCARD, SR.MAX_CONTAINMENT
COMPONENTS, GREEDY = 0, 1
UNDECIDED, REP, MEMBER = 0, 1, 2


def graph(sketches, metric, threshold, threshold_common=0):
    """the adjacency of the rule: u ~ v iff the pair is reported by the thresholded search"""
    if metric not in (JACCARD, MAX_CONTAINMENT):
        raise ValueError("clustering takes the symmetric metrics only")
    sets = [set(s) for s in sketches]
    owners = {}
    for v, s in enumerate(sets):
        for h in s:
            owners.setdefault(h, []).append(v)
    common = {}
    for held_by in owners.values():                 # only pairs that share a hash can be adjacent
        for i in range(len(held_by)):
            for j in range(i + 1, len(held_by)):
                key = (held_by[i], held_by[j])
                common[key] = common.get(key, 0) + 1
    adj = [dict() for _ in sets]
    for (v, u), c in common.items():
        if SR.reported(metric, threshold, threshold_common, c, len(sets[v]), len(sets[u])):
            value = SR.value(metric, c, len(sets[v]), len(sets[u]))
            adj[v][u] = (value, c)
            adj[u][v] = (value, c)
    return adj


def priority(scores):
    """the nodes in priority order: score descending, ties to the lower node"""
    return sorted(range(len(scores)), key=lambda v: (-scores[v], v))


def number(representative):
    """cluster[v]: clusters numbered 0, 1, ... in ascending order of their smallest member node"""
    ids, cluster = {}, []
    for v in range(len(representative)):
        r = representative[v]
        if r not in ids:
            ids[r] = len(ids)
        cluster.append(ids[r])
    return cluster, len(ids)


def components(adj, scores):
    """(cluster, representative, n_clusters) of single linkage"""
    n = len(adj)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    for v in range(n):
        for u in adj[v]:
            a, b = find(v), find(u)
            if a != b:
                parent[max(a, b)] = min(a, b)
    first = {}
    for v in priority(scores):                      # the first member of a component met in priority order represents it
        first.setdefault(find(v), v)
    representative = [first[find(v)] for v in range(n)]
    cluster, k = number(representative)
    return cluster, representative, k


def greedy_representatives(adj, scores):
    """the sequential rule: walk the nodes in priority order; v becomes a representative iff no earlier one is adjacent"""
    reps = set()
    for v in priority(scores):
        if not any(u in reps for u in adj[v]):
            reps.add(v)
    return reps


def greedy_rounds(adj, scores):
    """the same set by synchronous rounds, each reading only the states of the round before: (representatives, rounds)"""
    n = len(adj)
    rank = [0] * n
    for p, v in enumerate(priority(scores)):
        rank[v] = p
    state, rounds = [UNDECIDED] * n, 0
    while UNDECIDED in state:
        nxt = list(state)
        for v in range(n):
            if state[v] != UNDECIDED:
                continue
            earlier = [state[u] for u in adj[v] if rank[u] < rank[v]]
            if REP in earlier:
                nxt[v] = MEMBER
            elif UNDECIDED not in earlier:
                nxt[v] = REP
        state, rounds = nxt, rounds + 1
    return {v for v in range(n) if state[v] == REP}, rounds


def greedy(adj, scores, sizes):
    """(cluster, representative, rep_common, n_clusters): every node that is no representative joins the adjacent
    representative with the greatest value, ties to the one earlier in priority"""
    n = len(adj)
    reps = greedy_representatives(adj, scores)
    rank = [0] * n
    for p, v in enumerate(priority(scores)):
        rank[v] = p
    representative, rep_common = [], []
    for v in range(n):
        if v in reps:
            representative.append(v)
            rep_common.append(sizes[v])
            continue
        best = None
        for u, (value, common) in adj[v].items():
            if u in reps and (best is None or value > best[0] or (value == best[0] and rank[u] < rank[best[1]])):
                best = (value, u, common)
        representative.append(best[1])
        rep_common.append(best[2])
    cluster, k = number(representative)
    return cluster, representative, rep_common, k


def cluster(sketches, metric, threshold, threshold_common=0, linkage=COMPONENTS, scores=None):
    """(cluster, representative, rep_common or None, n_clusters) as smh_index_cluster writes them"""
    sizes = [len(set(s)) for s in sketches]
    scores = sizes if scores is None else list(scores)
    adj = graph(sketches, metric, threshold, threshold_common)
    if linkage == COMPONENTS:
        c, r, k = components(adj, scores)
        return c, r, None, k
    if linkage == GREEDY:
        return greedy(adj, scores, sizes)
    raise ValueError("unknown linkage")
