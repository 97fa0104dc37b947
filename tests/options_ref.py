"""The whole of Retriever.search_batch on the CPU: the oracles of the single options composed into one chain (imported by
test_options_ref.py and test_gpu_options_oracle.py).  No device code, no DeviceEngine.

    plans(c, batch)                        the batch's queries after the text syntax: one Plan per query
    without(plan, feature)                 the same query with ONE feature of options_cases.FEATURES taken away
    evaluate(c, plan, mode, diversify)     the expected result of one query (a dict, see evaluate)
    expected(c, batch, mode, diversify)    evaluate for every query of the batch
    bm25_search(c, batch, q)               what the BM25.search facade returns for the query: [(doc_id, score)]

IMPORTED as it is, because none of it decides which documents, terms or counts come out: the host text layer --
text.preprocess_query, text.simple_tokenize, text.extract_domain_topic (the rows' "domain" key, which facet_by="domain" groups
by), query.parse_queries (pinned by tests/golden/query_parse_cases.json), snippets.render, docset.url_host.
RESTATED from the documented contract (query.SearchOptions, DESIGN K8 - K18, include/msretr.h) and not from retriever.py: which
words are corrected and into what (fuzzy_ref), how patterns expand and where the expansion stops (wildcard_ref), the set a query
is restricted to (term_set_ref, phrase_ref, proximity_ref), what the facets count (facet_ref), stage 1 in either mode
(within_ref, hybrid_ref), the rerank chain (oracle_engine, oracle.rerank_ref), the collapse and its passive pages (dedup_ref),
diversification (oracle.rerank_ref), the snippet's query row, weights and window (snippet_ref), matched_by and duplicates."""
import math
import re
from dataclasses import dataclass, field, replace
from urllib.parse import urlparse

import numpy as np
import torch

import dedup_ref
import facet_ref
import fuzzy_ref
import hybrid_ref
import snippet_ref
import wildcard_ref
from msretr.docset import url_host
from msretr.query import Conditions, SearchOptions, parse_queries
from msretr.snippets import render
from msretr.text import Near, extract_domain_topic, preprocess_query, simple_tokenize
from oracle import rerank_ref
from oracle_engine import OracleEngine
from phrase_ref import phrase_mask_fast
from proximity_ref import near_mask_fast
from term_set_ref import term_set_mask
from within_ref import bm25_full

MAX_QUERY_TERMS = 64         # MSR_MAX_QUERY_TERMS (include/msretr.h)
MAX_ROW_TERMS = 16           # MSR_PHRASE_MAX_TERMS: the terms of a snippet's query row
SIG_WORDS, SHINGLE = 64, 4   # MSR_SIG_WORDS; the shingle width of the retriever's signatures (DESIGN K18)
MAX_WORD = 32                # MSR_FUZZY_MAX_LEN = MSR_WILD_MAX_LEN
MAX_CODE_POINT = 0xFFFE
RERANK_TOP_K, SMOOTHING, RERANK_MAX_DOCS = 100, 0.15, 1000   # reranker/config.yaml; the engine's default candidate rows
SRC_NAME = {1: "lexical", 2: "dense", 3: "both"}


@dataclass(frozen=True)
class Plan:
    """One query after the text syntax.  terms: the scoring terms (strings); must / must_not: terms; must_phrases /
    must_not_phrases: lists of terms or text.Near over a list of terms; patterns: lower-cased; within: bool [N] or None."""
    scoring: str
    terms: tuple
    vector: np.ndarray = field(compare=False, repr=False)
    must: tuple = ()
    must_not: tuple = ()
    must_phrases: tuple = ()
    must_not_phrases: tuple = ()
    patterns: tuple = ()
    within: np.ndarray = field(default=None, compare=False, repr=False)
    fuzzy: bool = False
    max_expansions: int = 8
    facets: tuple = None     # (facet_by, facet_limit)
    collapse: float = None   # duplicate_threshold
    snippets: int = None     # snippet_tokens
    top_k: int = 1000
    dense_k: int = 100


def plans(c, batch, preprocess=True):
    """preprocess=False: the texts as they are (the BM25.search facade appends no city) and a query without a scoring token
    and without a pattern loses its conditions (parse_queries' drop_empty)."""
    from options_cases import masks, vectors
    sw = batch.switches
    opts = SearchOptions(operators=sw.get("operators", False), phrases=sw.get("phrases", False), proximity=sw.get("proximity", False),
                         wildcards=sw.get("wildcards", False))
    given = lambda k: batch.lists.get(k)
    explicit = Conditions(given("must"), given("must_not"), given("must_phrases"), given("must_not_phrases"))
    texts = [preprocess_query(q) if preprocess else q for q in batch.queries]
    scoring, _, cond, pats = parse_queries(texts, simple_tokenize, opts, explicit, given("patterns"), drop_empty=not preprocess)
    Q, qv, within = len(texts), vectors(c, batch), masks(c, batch)
    of = lambda lists, q: () if lists is None else tuple(lists[q])
    phrase = lambda p: p.with_terms(simple_tokenize(p.terms)) if isinstance(p, Near) and isinstance(p.terms, str) else \
        p if isinstance(p, Near) else tuple(p)
    out = []
    for q in range(Q):
        terms = batch.term_lists[q] if batch.term_lists is not None and preprocess else simple_tokenize(scoring[q])
        out.append(Plan(scoring[q], tuple(terms), qv[q], of(cond.must, q), of(cond.must_not, q),
                        tuple(phrase(p) for p in of(cond.must_phrases, q)), tuple(phrase(p) for p in of(cond.must_not_phrases, q)),
                        of(pats, q), within[q], bool(sw.get("fuzzy")), int(sw.get("max_expansions", 8)),
                        (sw.get("facet_by", "host"), int(sw.get("facet_limit", 10))) if sw.get("facets") else None,
                        float(sw.get("duplicate_threshold", 0.9)) if sw.get("collapse_duplicates") else None,
                        int(sw.get("snippet_tokens", 30)) if sw.get("snippets") else None,
                        int(sw.get("top_k", 1000)), int(sw.get("dense_k", 100))))
    return out


def features_on(plan, c):
    """The features of options_cases.FEATURES a plan could exercise: its conditions, and the switches that are on."""
    near = [p for p in plan.must_phrases + plan.must_not_phrases if isinstance(p, Near)]
    vocab = c.ix.vocab
    on = {"within": plan.within is not None, "must": bool(plan.must), "must_not": bool(plan.must_not),
          "must_phrase": any(not isinstance(p, Near) for p in plan.must_phrases),
          "must_not_phrase": any(not isinstance(p, Near) for p in plan.must_not_phrases),
          "near_ordered": any(p.ordered for p in near), "near_unordered": any(not p.ordered for p in near),
          "fuzzy": plan.fuzzy and any(isinstance(t, str) and t not in vocab for t in plan.terms + plan.must),
          "wildcard": bool(plan.patterns), "facets_host": plan.facets is not None and plan.facets[0] == "host",
          "facets_domain": plan.facets is not None and plan.facets[0] == "domain", "collapse": plan.collapse is not None,
          "snippets": plan.snippets is not None}
    return {k for k, v in on.items() if v}


def without(plan, feature):
    near = lambda ps, ordered: tuple(p for p in ps if not (isinstance(p, Near) and p.ordered == ordered))
    exact = lambda ps: tuple(p for p in ps if isinstance(p, Near))
    change = {"within": dict(within=None), "must": dict(must=()), "must_not": dict(must_not=()),
              "must_phrase": dict(must_phrases=exact(plan.must_phrases)),
              "must_not_phrase": dict(must_not_phrases=exact(plan.must_not_phrases)),
              "near_ordered": dict(must_phrases=near(plan.must_phrases, True), must_not_phrases=near(plan.must_not_phrases, True)),
              "near_unordered": dict(must_phrases=near(plan.must_phrases, False), must_not_phrases=near(plan.must_not_phrases, False)),
              "fuzzy": dict(fuzzy=False), "wildcard": dict(patterns=()), "facets_host": dict(facets=None),
              "facets_domain": dict(facets=None), "collapse": dict(collapse=None), "snippets": dict(snippets=None)}
    return replace(plan, **change[feature])


# ------------------------------------------------------------------------------------------------ tables of a crawl, built once
class _Tables:
    def __init__(self, c):
        ix = c.ix
        self.N, self.V = ix.n_docs, ix.n_terms
        self.names = c.names
        self.df = np.diff(np.asarray(c.z["term_off"], np.int64))
        look = lambda s: isinstance(s, str) and 1 <= len(s) <= MAX_WORD and max(map(ord, s)) <= MAX_CODE_POINT
        self.lookable = look
        self.weights = [int(self.df[t]) if look(s) else 0 for t, s in enumerate(self.names)]        # never suggested at weight 0
        self.sig = dedup_ref.signatures_fast(c.off, c.tok, SHINGLE)
        urls, titles, texts = ix.urls, ix.titles, ix.texts
        self.rejected = np.asarray([urls[d] is None or titles[d] is None or texts[d] is None for d in range(self.N)], bool)
        self.domain_table = np.where(self.rejected, -1, 0).astype(np.int32)      # (the collapse reads the sign only)
        self.netloc = [None if urls[d] is None else urlparse(urls[d]).netloc.lower() for d in range(self.N)]
        self.facet = {}
        for by, key in (("host", url_host), ("domain", lambda u: None if url_host(u) is None else extract_domain_topic(u))):
            ids, value = {}, np.full(self.N, -1, np.int32)
            for d, u in enumerate(urls):
                k = key(u)
                if k is not None:
                    value[d] = ids.setdefault(k, len(ids))
            self.facet[by] = (value, list(ids))
        self.engine = OracleEngine(ix)
        self.doc_ids = np.asarray(c.z["doc_ids"])
        self._fuzzy, self._wild = {}, {}

    def fuzzy(self, word):
        """The nearest vocabulary term of an unknown word under the AUTO tolerance, or -1."""
        if word not in self._fuzzy:
            n = len(word)
            edits = 0 if n < 3 else 1 if n < 6 else 2
            got = -1
            if self.lookable(word) and edits > 0:
                term, _, cnt, _ = fuzzy_ref.expected(self.names, self.weights, [word], [edits], 1)
                got = int(term[0, 0]) if cnt[0] else -1
            self._fuzzy[word] = got
        return self._fuzzy[word]

    def wildcard(self, pattern, limit):
        if (pattern, limit) not in self._wild:
            term, n, total = wildcard_ref.expected(self.names, self.weights, [pattern], limit)
            self._wild[pattern, limit] = ([int(t) for t in term[0, :n[0]]], int(total[0]))
        return self._wild[pattern, limit]


_tables = {}


def tables(c):
    if id(c) not in _tables:
        _tables[id(c)] = _Tables(c)
    return _tables[id(c)]


# ------------------------------------------------------------------------------------------------ the stages
def term_ids(c, terms):
    return [int(t) if isinstance(t, (int, np.integer)) else c.ix.vocab.get(t, -1) for t in terms]


def correct(c, plan):
    """Ids: -> (scored ids, must ids, corrections {typed: used}).  Unknown scoring and must words are corrected; must_not,
    phrases and patterns never are."""
    T = tables(c)
    corrections = {}

    def fix(terms):
        out = []
        for t, i in zip(terms, term_ids(c, terms)):
            if i < 0 and plan.fuzzy and isinstance(t, str):
                j = T.fuzzy(t)
                if j >= 0:
                    i, corrections[t] = j, T.names[j]
            out.append(i)
        return out
    return fix(plan.terms), fix(plan.must), corrections


def expand(c, plan, ids):
    """Expansion: -> (scored ids, expansions).  A query may hold MSR_MAX_QUERY_TERMS distinct entries, and an unknown word (-1)
    is an entry: DeviceEngine.pack_queries packs it as a term and refuses a query of more, which is what decided the point
    the contract left open (SearchOptions, wildcards=True).  So: every pattern once, in order; a match the query already
    holds is named and not added; a new match is added while the DISTINCT entries of the query, counted afresh, are below
    the limit; the first one that finds the query full ends its pattern as "truncated"."""
    T = tables(c)
    query, info = list(ids), {}
    for p in dict.fromkeys(plan.patterns):
        if not T.lookable(p) or len(p.replace("*", "").replace("?", "")) < 2:
            info[p] = {"terms": [], "total": 0, "skipped": True}
            continue
        found, total = T.wildcard(p, plan.max_expansions)
        info[p] = {"terms": [], "total": total}
        for t in found:
            if t not in query:
                if len(set(query)) >= MAX_QUERY_TERMS:
                    info[p]["truncated"] = True
                    break
                query.append(t)
            info[p]["terms"].append(T.names[t])
    return query, info


def the_set(c, plan, must_ids):
    """The set: within AND the required terms AND NOT the excluded ones AND every required phrase / window AND NOT any
    excluded one.  None: no restriction at all."""
    T = tables(c)
    if plan.within is None and not (plan.must or plan.must_not or plan.must_phrases or plan.must_not_phrases):
        return None
    mask = term_set_mask(c.z, must_ids, term_ids(c, plan.must_not), plan.within)

    def holds(p):
        if isinstance(p, Near):
            ids = term_ids(c, p.terms)
            span = (len(ids) if p.ordered else len(set(ids))) + p.slop
            return near_mask_fast(c.off, c.tok, ids, span, p.ordered, None, T.V)
        return phrase_mask_fast(c.off, c.tok, term_ids(c, p), None, T.V)
    for p in plan.must_phrases:
        mask = mask & holds(p)
    for p in plan.must_not_phrases:
        mask = mask & ~holds(p)
    return mask


def facets(c, plan, ids, mask):
    """-> (hits, [{"value", "count"}], distinct values hit): counted over every page of the set that holds a counting term."""
    T = tables(c)
    by, limit = plan.facets
    valid = list(dict.fromkeys(t for t in ids if 0 <= t < T.V))
    counting = [t for t in valid if float(c.z["idf"][t]) > 0] or valid
    if not counting:
        return 0, [], 0
    value, names = T.facet[by]
    hits, cnt, top = facet_ref.brute_force(c.z, value, len(names), counting, mask, limit)
    return hits, [{"value": names[v], "count": n} for v, n in top], len(cnt)


def stage1(c, plan, ids, mask, mode):
    """-> (doc int64, score f64, src int32) candidates of one query: lexical, the BM25 list inside the set cut to top_k;
    hybrid, the BM25 top k_lex and the dense top dense_k inside the set."""
    if mode == "hybrid":
        return hybrid_ref.candidates(c.z, c.ix.emb, c.ix.doc_off, ids, plan.vector, plan.top_k, RERANK_MAX_DOCS, plan.dense_k,
                                     c.ix.k1, c.ix.b, mask)
    fd, fs = bm25_full(c.z, ids, 0.0, c.ix.k1, c.ix.b)
    if mask is not None:
        keep = mask[fd]
        fd, fs = fd[keep], fs[keep]
    return fd[:plan.top_k], fs[:plan.top_k], np.ones(min(len(fd), plan.top_k), np.int32)


def fuse(c, plan, doc, score):
    """Rerank: the gather's cosines and the fuse of oracle.rerank_ref -> (doc, score, orig, chunk) arrays of the fused list."""
    T = tables(c)
    M = max(len(doc), 1)
    cd, cs = np.full((1, M), -1, np.int32), np.full((1, M), -np.inf)
    cd[0, :len(doc)], cs[0, :len(doc)] = doc, score
    cn = np.asarray([len(doc)], np.int32)
    cos, meta = T.engine.rerank_gather(torch.as_tensor(np.asarray(plan.vector, np.float32)[None, :]), cd, cn)
    fd, fs, fo, fc, fn, _ = [x.numpy() for x in T.engine.rerank_fuse(cd, cs, cn, cos, meta, smoothing=SMOOTHING)]
    n = int(fn[0])
    return fd[0, :n], fs[0, :n], fo[0, :n], fc[0, :n]


def collapse(c, plan, fused, passive=True):
    """Collapse: -> (the fused list without the dropped rows, drops [(doc, leader, matches)] in drop order).  passive=False:
    the WRONG collapse that lets a rejected page lead and drop (test_options_ref.py: the cases must tell the two apart)."""
    T = tables(c)
    mm = int(math.ceil(plan.collapse * SIG_WORDS))
    n = len(fused[0])
    if n == 0:
        return fused, []
    out = dedup_ref.collapse_lists(*(np.asarray(x)[None, :] for x in fused), np.asarray([n], np.int32), T.sig, mm, T.domain_table if passive else None)
    k, nd = int(out[4][0]), int(out[8][0])
    return tuple(o[0, :k] for o in out[:4]), [(int(out[5][0, j]), int(out[6][0, j]), int(out[7][0, j])) for j in range(nd)]


def diversified(c, fused, diversify, top=RERANK_TOP_K):
    """Diversify: the accepted rows (a page without a urlsDB row or with a NULL title, url or text never appears) through
    oracle.rerank_ref.hybrid_diversification, or the first `top` of them (the reranker's top_k) -> [(doc, score)]."""
    T = tables(c)
    items = [{"doc": int(d), "url": c.ix.urls[int(d)], "similarity_score": float(s)} for d, s in zip(fused[0], fused[1])
             if not T.rejected[int(d)]]
    out = rerank_ref.hybrid_diversification(items, top_k=top) if diversify else items[:top]
    return [(x["doc"], x["similarity_score"]) for x in out]


def snippets(c, plan, ids, docs):
    """Snippets: per final row (snippet or None, highlights, missing).  The query row: the distinct scored terms (at most
    MSR_PHRASE_MAX_TERMS: the heaviest stay, of equal ones the earlier), weights max(1, min(MSR_SNIPPET_MAX_WEIGHT, round(1024 *
    max(idf, 0))))."""
    T = tables(c)
    weight = lambda t: max(1, min(snippet_ref.WMAX, round(1024 * max(float(c.z["idf"][t]), 0.0))))
    row = list(dict.fromkeys(t for t in ids if 0 <= t < T.V))
    if len(row) > MAX_ROW_TERMS:
        keep = sorted(sorted(range(len(row)), key=lambda j: (-weight(row[j]), j))[:MAX_ROW_TERMS])
        row = [row[j] for j in keep]
    names = [T.names[t] for t in row]
    if not row or not docs:
        return [(None, [], list(names)) for _ in docs]
    span = int(plan.snippets)
    start, _, _, mask, bits = snippet_ref.best_windows_fast(c.off, c.tok, docs, [0] * len(docs), [row], [[weight(t) for t in row]],
                                                            [span], T.V)
    out = []
    for i, d in enumerate(docs):
        if start[i] < 0:
            out.append((None, [], list(names)))
            continue
        text, hl = render(c.ix.titles[d], c.ix.texts[d], int(start[i]), int(mask[i]), span)
        out.append((text, hl, [w for j, w in enumerate(names) if not int(bits[i]) >> j & 1]))
    return out


_WORD = re.compile(r"\w+", re.UNICODE)


def evaluate(c, plan, mode="lexical", diversify=True, rerank_top=RERANK_TOP_K, passive=True):
    """-> {"rows": [{"doc", "doc_id", "score", "snippet", ("matched_by"), ("duplicates"), ("highlights", "missing")}],
    "collapsed", "corrections", "corrected_query", "expansions", "hits", "facets", "facet_values"} and, for the checks on the
    oracle itself, "set" (bool [N] or None), "fused" (docs, scores before the collapse), "drops", "scored" (ids), "dense_gap"."""
    T = tables(c)
    ids, must_ids, corrections = correct(c, plan)
    ids, expansions = expand(c, plan, ids)
    mask = the_set(c, plan, must_ids)
    hits, top, n_values = facets(c, plan, ids, mask) if plan.facets is not None else (None, [], 0)
    doc, score, src = stage1(c, plan, ids, mask, mode)
    fused = fuse(c, plan, doc, score)
    kept, drops = collapse(c, plan, fused, passive) if plan.collapse is not None else (fused, [])
    final = diversified(c, kept, diversify, rerank_top)
    docs = [d for d, _ in final]
    source = dict(zip((int(d) for d in doc), (int(s) for s in src)))
    led = {}
    ix = c.ix
    for d, lead, m in drops:
        led.setdefault(lead, []).append({"doc_id": str(int(T.doc_ids[d])), "url": ix.urls[d], "title": ix.titles[d] or "No Title",
                                         "similarity": m / 64.0})
    passages = snippets(c, plan, ids, docs) if plan.snippets is not None else None
    rows = []
    for r, (d, s) in enumerate(final):
        text = ix.texts[d]
        row = {"doc": d, "doc_id": str(int(T.doc_ids[d])), "score": s,
               "snippet": (text[:200] + "..." if len(text) > 200 else text) or "No content available"}
        if mode == "hybrid":
            row["matched_by"] = SRC_NAME[source[d]]
        if d in led:
            row["duplicates"] = led[d]
        if passages is not None:
            if passages[r][0] is not None:
                row["snippet"] = passages[r][0]
            row["highlights"], row["missing"] = passages[r][1], passages[r][2]
        rows.append(row)
    corrected = _WORD.sub(lambda m: corrections.get(m.group(0).lower(), m.group(0)), plan.scoring) if corrections else None
    return {"rows": rows, "collapsed": len(drops), "corrections": corrections, "corrected_query": corrected,
            "expansions": expansions, "hits": hits, "facets": top, "facet_values": n_values,
            "set": mask, "fused": (fused[0].tolist(), fused[1].tolist()), "drops": drops, "scored": ids,
            "dense_gap": dense_gap(c, plan, mask) if mode == "hybrid" else None}


def dense_gap(c, plan, mask):
    """The cosine margin between the last dense candidate and the first page left out (inf: the set holds no more)."""
    from oracle import dense_ref
    best, _ = dense_ref.doc_scores(c.ix.emb, c.ix.doc_off, plan.vector)
    ok = np.isfinite(best) if mask is None else np.isfinite(best) & mask
    top = np.sort(best[ok].astype(np.float64))[::-1]
    return float(top[plan.dense_k - 1] - top[plan.dense_k]) if len(top) > plan.dense_k else float("inf")


PUBLIC = ("rows", "collapsed", "corrections", "corrected_query", "expansions", "hits", "facets", "facet_values")


def public(result):
    """What a caller sees of evaluate's answer (the comparison of the no-vacuous-case condition)."""
    return {k: result[k] for k in PUBLIC}


def expected(c, batch, mode="lexical", diversify=True, rerank_top=RERANK_TOP_K):
    return [evaluate(c, p, mode, diversify, rerank_top) for p in plans(c, batch)]


def bm25_search(c, batch, q):
    """BM25.search(text, ...) for query q of the batch, the text as it is: the BM25 list inside the set, cut to top_k, then
    without the pages that have no urlsDB row -> ([(doc_id, score)], corrections, expansions)."""
    T = tables(c)
    plan = plans(c, batch, preprocess=False)[q]
    if not plan.terms and not plan.patterns:
        return [], {}, {}
    ids, must_ids, corrections = correct(c, plan)
    mask = the_set(c, plan, must_ids)
    ids, expansions = expand(c, plan, ids)
    doc, score, _ = stage1(c, plan, ids, mask, "lexical")
    return [(int(T.doc_ids[d]), float(s)) for d, s in zip(doc, score) if c.ix.urls[d] is not None], corrections, expansions
