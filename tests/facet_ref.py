"""Shared cases and the plain numpy reference of the facet counts (msr_facet_counts, DESIGN K17).

    facet_counts_ref(z, value, n_values, any, base_mask) -> (hits, counts int64 [n_values])     np.bincount over the match mask
    top_ref(counts, limit) -> (values, counts, n_values_hit)                                     (count desc, value asc)
    brute_force(...)                                                                             the same with python dicts
    table_ref(value, n_values) -> the five arrays of msr_facet_table, restated in numpy
    value_layouts(N) -> [(name, value int32 [N], n_values)]
    facet_rows(c) -> [(any term ids, row_base, claim)]

The corpora, their named terms and their base rows are term_set_ref's (K11): the sizes straddle a bitset word, a skip-table
tile and the kernel's span S."""
import numpy as np

from term_set_ref import BIG, S, SIZES, base_mask, corpus, term_set_mask  # noqa: F401  (re-exported for the tests)


def match_mask(z, any_terms, base=None):
    """bool [N]: base AND (OR of the terms' documents); an empty list is no term condition; a term outside [0, n_terms) or with
    an empty list contributes nothing."""
    N = int(z["n_docs"])
    if len(any_terms) == 0:
        m = np.ones(N, bool)
    else:
        m = np.zeros(N, bool)
        for t in set(int(t) for t in any_terms):
            m |= term_set_mask(z, [t], [], None)
    return m if base is None else m & np.asarray(base, bool)


def facet_counts_ref(z, value, n_values, any_terms, base=None):
    m = match_mask(z, any_terms, base)
    sel = np.asarray(value)[m]
    return int(m.sum()), np.bincount(sel[sel >= 0], minlength=int(n_values)).astype(np.int64)


def top_ref(counts, limit):
    """-> (values int32 [limit] padded with -1, counts int32 [limit] padded with 0, number of values with count > 0)."""
    counts = np.asarray(counts, np.int64)
    order = np.lexsort((np.arange(len(counts)), -counts))
    order = order[counts[order] > 0]
    tv, tc = np.full(limit, -1, np.int32), np.zeros(limit, np.int32)
    k = min(limit, len(order))
    tv[:k], tc[:k] = order[:k], counts[order[:k]]
    return tv, tc, int(len(order))


def brute_force(z, value, n_values, any_terms, base=None, limit=10):
    """-> (hits, {value: count}, top list [(value, count)]) with python sets and dicts, document by document."""
    off, post = [int(v) for v in z["term_off"]], [int(v) for v in z["post_doc"]]
    V, N = len(off) - 1, int(z["n_docs"])
    if len(any_terms) == 0:
        docs = set(range(N))
    else:
        docs = set()
        for t in any_terms:
            if 0 <= t < V:
                docs |= set(post[off[t]:off[t + 1]])
    if base is not None:
        docs = {d for d in docs if base[d]}
    cnt = {}
    for d in docs:
        v = int(value[d])
        if v >= 0:
            cnt[v] = cnt.get(v, 0) + 1
    top = sorted(cnt.items(), key=lambda kv: (-kv[1], kv[0]))[:limit]
    return len(docs), cnt, top


def table_ref(value, n_values):
    """msr_facet_table's contract in numpy -> (local uint16 [N], span_off, span_values, value_off, value_pos), int32."""
    value = np.asarray(value, np.int64)
    N = len(value)
    local = np.full(N, 0xFFFF, np.uint16)
    span_off, span_values = [0], []
    for d0 in range(0, N, S):
        v = value[d0:d0 + S]
        u = np.unique(v[v >= 0])
        local[d0:d0 + S][v >= 0] = np.searchsorted(u, v[v >= 0])
        span_values.append(u)
        span_off.append(span_off[-1] + len(u))
    span_values = np.concatenate(span_values) if span_values else np.zeros(0, np.int64)
    value_pos = np.argsort(span_values, kind="stable")       # per value its slots, ascending
    value_off = np.concatenate([[0], np.cumsum(np.bincount(span_values, minlength=n_values))])
    i32 = lambda a: np.asarray(a, np.int32)
    return local, i32(span_off), i32(span_values), i32(value_off), i32(value_pos)


def value_layouts(N):
    rng = np.random.default_rng(77 + N)
    d = np.arange(N)
    L = [("one value", np.zeros(N, np.int32), 1),                        # a span's slot counts exactly S in 16 bits
         ("own value", d.astype(np.int32), N),                           # local ids up to S - 1, a full dictionary
         ("no value", np.full(N, -1, np.int32), 3)]
    v = (d % 3).astype(np.int32)
    v[::7] = -1
    L.append(("mod 3, every 7th none", v, 3))
    alive = rng.permutation(300)[:250]                                   # 50 values no document has
    w = 1.0 / (1.0 + np.arange(250)) ** 1.3
    L.append(("skewed over 300", alive[rng.choice(250, N, p=w / w.sum())].astype(np.int32), 300))
    v = (d % 4).astype(np.int32)
    v[((N - 1) // 32) * 32:] = 4
    L.append(("a value only in the last word", v, 6))
    if N > 2 * S:
        v = (d % 5).astype(np.int32)
        v[2 * S::2] = 5
        L.append(("a value only in span 2", v, 6))
    return L


def facet_rows(c):
    """(any list, row_base, claim): every list with base -1, with each base row and with an out-of-range base."""
    t, V, nb = c.term, len(c.term), len(c.bases)
    lists = [([], "empty list: no term condition")]
    for n in ("all", "even", "empty", "rnd1", "skipper", "n2047", "n2048", "last_word"):
        if n in t:
            lists.append(([t[n]], n))
    for d in (0, 31, 32, 1023, 1024, S - 1, S):
        if f"one_{d}" in t:
            lists.append(([t[f"one_{d}"]], f"one posting at document {d}"))
    lists.append(([V + 5, -3, t["even"], t["even"], t["rnd1"]], "an id out of range, a negative id, a repeated id"))
    pool = [t[n] for n in ("rnd1", "empty", "one_0", "one_last", "last_word") if n in t] + [-1, V]
    lists.append(([pool[i % len(pool)] for i in range(300)], "300 terms: more than one round of searches"))
    return [(a, b, f"{claim}, base {b}") for a, claim in lists for b in [-1] + list(range(nb)) + [nb]]
