"""Site facets and hit counts (DESIGN K17): which sites a query matches, how many pages each has, how many pages match at all.

    value, names = facet_values(ix)                          # one int32 per document: its host's id, -1 = none
    engine.bind_facet(value, len(names))
    hits, n_hit, top_value, top_count = engine.facet_counts(term_lists, within=..., limit=10)
    retriever.search(query, facets=True)                     # .hits, .facets, .facet_values on the result

The counts are taken on the device over the WHOLE match set (msr_facet_counts), not over the ~100 rows a result list is cut to.
"""
import ctypes as C

import numpy as np

from . import _abi
from .docset import _host_table, url_host
from .text import extract_domain_topic

FACET_KEYS = ("host", "domain")


def facet_values(ix, by="host"):
    """-> (value int32 [N], names): value[d] indexes names, -1 for a document without a URL or without a host.
    by="host" (default): docset.url_host through docset's host table -- a facet value can be handed back as sites=[...].
    by="domain": text.extract_domain_topic(url), the "domain" key the result rows already carry.
    Both are built once per index and kept on it while its `urls` list is the same object of the same length.  An index
    without URLs raises ValueError, as does any other `by`."""
    if by not in FACET_KEYS:
        raise ValueError(f"facet_by must be one of {FACET_KEYS} (got {by!r})")
    if ix.urls is None:
        raise ValueError("facets need an index with URLs (CorpusIndex.urls)")
    if by == "host":
        value, hosts = _host_table(ix)
        return value, hosts
    urls = ix.urls
    got = getattr(ix, "_facet_domains", None)
    if got is not None and got[0] is urls and got[1] == len(urls):
        return got[2], got[3]
    ids, names = {}, []
    value = np.full(len(urls), -1, np.int32)
    for i, u in enumerate(urls):
        if url_host(u) is None:
            continue
        name = extract_domain_topic(u)
        j = ids.get(name)
        if j is None:
            j = ids[name] = len(names)
            names.append(name)
        value[i] = j
    ix._facet_domains = (urls, len(urls), value, names)
    return value, names


def check_options(facet_by, facet_limit):
    """ValueError unless facet_by is a key of FACET_KEYS and facet_limit an int of 1 .. MSR_FACET_MAX_LIMIT."""
    if isinstance(facet_limit, bool) or not isinstance(facet_limit, (int, np.integer)) or \
            not 1 <= int(facet_limit) <= _abi.MSR_FACET_MAX_LIMIT:
        raise ValueError(f"facet_limit must be 1 .. MSR_FACET_MAX_LIMIT = {_abi.MSR_FACET_MAX_LIMIT} (got {facet_limit!r})")
    if facet_by not in FACET_KEYS:
        raise ValueError(f"facet_by must be one of {FACET_KEYS} (got {facet_by!r})")


def build_table(value, n_values):
    """msr_facet_table: value int32 [N] in [-1, n_values) -> (local uint16 [N], span_off int32 [n_spans + 1], span_values int32
    [T], value_off int32 [n_values + 1], value_pos int32 [T]), the per-span dictionaries msr_bind_facet takes (msretr.h).  Two
    calls: the first only counts T.  ValueError for a value outside [-1, n_values)."""
    lib = _abi.load()
    value = np.ascontiguousarray(value, np.int32)
    N, n_values = int(value.shape[0]), int(n_values)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    T = int(lib.msr_facet_table(p(value), N, n_values, None, None, None, None, None))
    if T < 0:
        raise ValueError(f"facet table: a value outside [-1, {n_values}) (msr_facet_table returned {T})")
    S = _abi.MSR_TERMSET_SPAN_DOCS
    local = np.empty(N, np.uint16)
    span_off = np.empty((N + S - 1) // S + 1, np.int32)
    span_values, value_pos = np.empty(T, np.int32), np.empty(T, np.int32)
    value_off = np.empty(n_values + 1, np.int32)
    got = int(lib.msr_facet_table(p(value), N, n_values, p(local), p(span_off), p(span_values), p(value_off), p(value_pos)))
    if got != T:
        raise _abi.MsrError(got, "msr_facet_table")
    return local, span_off, span_values, value_off, value_pos


def counting_terms(ix, ids):
    """The term ids whose documents a query's facets count: the query's unique valid ids (in [0, n_terms), first occurrence
    first) with idf > 0.  A term with idf <= 0 -- the city term that preprocessing appends to every query -- cannot lift a page
    over min_score = 0 on its own, and counting it would make every facet list the corpus's.  If NO term has a positive idf,
    all valid terms count.  A query without a valid term gets [] -- it has 0 hits, and no device call is made for it.
    What the numbers then mean: `hits` is the number of pages that hold AT LEAST ONE counting term inside the restriction
    (within=, operators, phrases, proximity); it is not the length of BM25's unlimited list under an arbitrary min_score."""
    n_terms = int(ix.n_terms)
    idf = ix.idf
    seen, valid = set(), []
    for t in ids:
        t = int(t)
        if 0 <= t < n_terms and t not in seen:
            seen.add(t)
            valid.append(t)
    positive = [t for t in valid if float(idf[t]) > 0]
    return positive or valid


def top_list(names, top_value, top_count):
    """One row of facet_counts' top arrays -> [{"value": name, "count": n}, ...]."""
    return [{"value": names[int(v)], "count": int(c)} for v, c in zip(top_value, top_count) if int(v) >= 0]
