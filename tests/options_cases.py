"""One small crawl and a covering table of queries with the query options on together (imported by options_ref.py's tests:
test_options_ref.py on the CPU, test_gpu_options_oracle.py on the GPU; test_gpu_query_options.py takes _word and _streams).

    crawl() -> Crawl           2400 pages with everything the options read, built once per process
    BATCHES                    four batches of eight queries; each query declares the FEATURES it exercises
    masks(c, batch)            the per-query `within` masks of a batch (from its site lists)
    vectors(c, batch)          its query vectors
    call_kwargs(c, batch, q)   the keywords of Retriever.search_batch (q=None) / Retriever.search (one query) for the batch

The corpus merges the `site` fixture of test_gpu_query_options.py with test_gpu_dedup's crawl: a vocabulary with term strings, a
forward index that agrees with the postings, hosts with a skewed distribution, pages without a URL (no urlsDB row) or without a
title (rejected by the response models), pages without tokens and without chunk rows, planted word pairs for phrases and
proximity, misspellable and wildcardable words, near-copies (one token differs; exact mirrors) under another scheme or host, and
one to four embedding rows per page.  A copy's embedding row is the page's plus noise of a quarter of its length (a page with
copies has ONE row: two boosted rows could both clamp at 1.0): the collapse is greedy in rank order, so a page and its copy
must not be near-tied, and the query vectors' seeds are chosen so that no two rows are (test_options_ref.py asserts the margin).
Of each topic with copies, six more pages fail exactly ONE condition of the everything-on cases and a seventh lies outside their
sites, so that every single condition decides about a page.

What "a feature is on in a query" means here.  fuzzy, wildcards, facets, collapse_duplicates and snippets are switches of a whole
search_batch call, and a batch also holds queries that cannot use them (a query of unknown words has nothing to collapse).  So
every query DECLARES the features it exercises, test_options_ref.py asserts of each declared feature that it is switched on and
that the oracle's answer changes when that one feature is taken away, and the pair table is counted over the declared features.
facets_host and facets_domain cannot be on together (facet_by is one value per call): that pair is the one exclusion."""
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

import dedup_ref
from msretr._abi import MSR_MAX_QUERY_TERMS
from msretr.docset import url_host
from msretr.index import _np
from msretr.index_build import idf_real
from msretr.text import Near

FEATURES = ("within", "must", "must_not", "must_phrase", "must_not_phrase", "near_ordered", "near_unordered", "fuzzy", "wildcard",
            "facets_host", "facets_domain", "collapse", "snippets")
EXCLUSIVE = {frozenset(("facets_host", "facets_domain"))}     # facet_by is one value per call


def _word(t):
    s, t = "", int(t)
    while True:
        s = chr(ord("a") + t % 26) + s
        t //= 26
        if t == 0:
            return "w" + s


def _streams(ix):
    """A forward index that agrees with the postings: every document's terms ascending, each tf times."""
    off, doc, tf = _np(ix.term_off).astype(np.int64), _np(ix.post_doc).astype(np.int64), _np(ix.post_tf).astype(np.int64)
    term = np.repeat(np.arange(len(off) - 1), np.diff(off))
    order = np.lexsort((term, doc))
    tok = np.repeat(term[order], tf[order]).astype(np.int32)
    lens = np.bincount(doc, weights=tf, minlength=ix.n_docs).astype(np.int64)
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), tok


# ------------------------------------------------------------------------------------------------ the crawl
N_DOCS, N_FILL = 2400, 1500
SEED = 2024
COPY_NOISE = 0.25            # a copy's embedding row = the page's (unit) row + COPY_NOISE * a unit-variance-per-row direction
HOSTS = ["uni-tuebingen.de", "www.tuebingen.de", "tuebingen.de", "example.org"] + [f"s{i}.example.net" for i in range(40)]
CITY = "tübingen"
TOPICS = ["mensa", "bibliothek", "semesterticket", "hochschulsport", "wohnheim"]      # 70 pages each
PLANTED = TOPICS[:3]                                         # ... the first 10 of theirs have two copies each
SIDE = ["universität", "unibibliothek", "bibliothekar", "bibliotheken"]                # 40 pages each: uni*, bib*
F = None                                                     # a filler slot of a planted sequence
# name -> (sequence, share of the pages that hold it)
PLANTS = {"essen": (["essen"], 0.7), "geschlossen": (["geschlossen"], 0.3),
          "alte aula": (["alte", "aula"], 0.6), "aula alte": (["aula", "alte"], 0.2), "alte . aula": (["alte", F, "aula"], 0.2),
          "kein zutritt": (["kein", "zutritt"], 0.3), "zutritt kein": (["zutritt", "kein"], 0.2),
          "morgens . abends": (["morgens", F, "abends"], 0.6), "abends . morgens": (["abends", F, "morgens"], 0.3),
          "morgens ... abends": (["morgens", F, F, F, "abends"], 0.2),
          "kuchen . kaffee": (["kuchen", F, "kaffee"], 0.6), "kaffee .... kuchen": (["kaffee", F, F, F, F, "kuchen"], 0.2)}
RICH = ("essen", "alte aula", "morgens . abends", "kuchen . kaffee")      # what a page with copies holds; it holds nothing else
NEARLY = ({"essen": False}, {"geschlossen": True}, {"alte aula": False, "aula alte": True}, {"kein zutritt": True},
          {"morgens . abends": False, "abends . morgens": True}, {"kuchen . kaffee": False, "kaffee .... kuchen": True})
NAMED = [CITY] + TOPICS + SIDE + sorted({w for seq, _ in PLANTS.values() for w in seq if w is not F})
BIG_SITES = ["tuebingen.de", "example.org", "s0.example.net", "s1.example.net", "s2.example.net"]      # most of the pages
UNI_SITES = ["uni-tuebingen.de", "example.org"]
NET_SITES = ["example.net"]


@dataclass
class Crawl:
    ix: object               # CorpusIndex on host arrays
    off: np.ndarray          # forward index
    tok: np.ndarray
    names: list              # term strings by id
    copies: dict             # page -> (print view, mirror)
    pages: dict              # topic word -> its own pages
    must_copy: tuple         # (page without "essen", its copy that holds it in the one token that differs)
    z: dict = field(default_factory=dict)
    rejected: tuple = ()     # pages with copies that the response models reject: (an original, its print view, another page's print view)


@lru_cache(maxsize=1)
def crawl():
    rng = np.random.default_rng(SEED)
    vocab = {w: i for i, w in enumerate(NAMED)}
    first = len(NAMED)
    for i in range(N_FILL):
        vocab[_word(first + i)] = first + i
    names = [None] * len(vocab)
    for w, t in vocab.items():
        names[t] = w
    assert len(set(names)) == len(names)
    fill_p = 1.0 / (1.0 + np.arange(N_FILL)) ** 0.7
    fill_p /= fill_p.sum()
    filler = lambda n: (first + rng.choice(N_FILL, n, p=fill_p)).tolist()
    flags = [{name: bool(rng.random() < p) for name, (_, p) in PLANTS.items()} for _ in range(N_DOCS)]
    words = [[] for _ in range(N_DOCS)]                      # single words a page holds beside its fillers
    free = list(rng.permutation(N_DOCS))
    pages = {}
    for w in TOPICS + SIDE:
        pages[w] = [int(free.pop()) for _ in range(70 if w in TOPICS else 40)]
        for p in pages[w]:
            words[p] += [w] * int(rng.integers(1, 4))
    for w in PLANTED:
        for p in pages[w][:10]:
            flags[p] = {name: name in RICH for name in PLANTS}
        flags[pages[w][16]] = {name: name in RICH for name in PLANTS}
        for p, change in zip(pages[w][10:16], NEARLY):       # six pages that fail ONE condition of the everything-on cases each
            flags[p] = dict({name: name in RICH for name in PLANTS}, **change)
    lone = pages["semesterticket"][20]                       # the page whose copy alone satisfies must=["essen"]
    flags[lone]["essen"] = False

    def page(d):
        segs = [[t] for t in filler(int(rng.integers(40, 91)))]
        if rng.random() < 0.85:
            segs += [[vocab[CITY]]] * int(rng.integers(1, 3))
        segs += [[vocab[w]] for w in words[d]]
        for name, (seq, _) in PLANTS.items():
            if flags[d][name]:
                segs.append([filler(1)[0] if w is F else vocab[w] for w in seq])
        return np.asarray([t for i in rng.permutation(len(segs)) for t in segs[i]], np.int32)
    streams = [page(d) for d in range(N_DOCS)]
    host = rng.choice(len(HOSTS), N_DOCS, p=(lambda w: w / w.sum())(1.0 / (1.0 + np.arange(len(HOSTS))) ** 1.2))
    for w in PLANTED:                                        # the six NEARLY pages lie inside BIG_SITES; a seventh holds everything
        #                                                      the everything-on cases ask for and lies outside them
        host[pages[w][10:16]] = HOSTS.index("example.org")
        host[pages[w][16]] = HOSTS.index("uni-tuebingen.de")
    rows = np.where(rng.random(N_DOCS) < 0.8, 1, rng.integers(2, 5, N_DOCS))
    copies, taken = {}, set()
    for w in PLANTED:
        for p in pages[w][:10]:
            a, b = int(free.pop()), int(free.pop())
            streams[a] = streams[p].copy()                   # the print view: the last token differs
            streams[a][-1] = first + (int(streams[a][-1]) - first + 1) % N_FILL if streams[a][-1] >= first else first
            streams[b] = streams[p].copy()                   # the mirror
            copies[p] = (a, b)
            taken |= {p, a, b}
    lone_copy = int(free.pop())
    streams[lone_copy] = streams[lone].copy()
    at = int(np.nonzero(streams[lone] >= first)[0][0])       # a filler token becomes the required word
    streams[lone_copy][at] = vocab["essen"]
    copies[lone] = (lone_copy,)
    taken |= {lone, lone_copy}
    empty = [int(free.pop()) for _ in range(5)]
    for d in empty:
        streams[d] = np.zeros(0, np.int32)
    chunkless = [int(free.pop()) for _ in range(3)]
    rows[chunkless] = 0
    rows[sorted(taken)] = 1                                  # one row: no positional boost, so a page and its copy never both clamp at 1.0
    ix, off, tok = dedup_ref.index_of(streams, len(vocab))
    ix.idf = idf_real(ix.total_docs, np.diff(np.asarray(ix.term_off, np.int64))).astype(np.float32)
    ix.vocab = vocab
    ids = _np(ix.doc_ids)
    url = lambda d: f"https://{HOSTS[host[d]]}/doc{int(ids[d])}"
    ix.urls = [None if d % 97 == 5 and d not in taken else url(d) for d in range(N_DOCS)]
    for p, cs in copies.items():
        ix.urls[cs[0]] = url(p).replace("https://", "http://") + "/print"            # the same host, another scheme and path
        if len(cs) > 1:
            ix.urls[cs[1]] = f"https://mirror.example.org/doc{int(ids[p])}"          # another host
    ix._url_group = None
    text = lambda s: " ".join(names[int(t)] for t in s)
    ix.titles = [text(streams[d][:3]) if d % 5 == 0 else "" for d in range(N_DOCS)]
    ix.texts = [text(streams[d][3:]) if d % 5 == 0 else text(streams[d]) for d in range(N_DOCS)]
    for d in range(N_DOCS):
        if d % 89 == 7 and d not in taken:
            ix.titles[d] = None                              # a page the response models reject
    # ... and among the pages with copies (the collapse must take them for passive: they neither lead nor drop): an original
    # AND its print view, so that the mirror is shown and swallows nothing; and the print view of another original, which
    # that original must not swallow.  The query vectors lean towards the first, so it ranks ahead of its copies.
    gone, kept = pages["mensa"][0], pages["mensa"][1]
    rejected = (gone, copies[gone][0], copies[kept][0])
    for d in rejected:
        ix.titles[d] = None
    doc_off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int32)
    emb = rng.standard_normal((int(doc_off[-1]), 768)).astype(np.float32)
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)
    for p, cs in copies.items():
        for c in cs:
            noise = rng.standard_normal((int(rows[p]), 768)).astype(np.float32) * np.float32(COPY_NOISE / np.sqrt(768))
            emb[doc_off[c]:doc_off[c + 1]] = emb[doc_off[p]:doc_off[p + 1]] + noise
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)
    ix.doc_off, ix.chunk_ids, ix.emb = doc_off, np.arange(len(emb), dtype=np.int64), emb
    z = {k: _np(getattr(ix, k)) for k in ("doc_ids", "doc_len", "term_off", "post_doc", "post_tf", "idf")}
    z.update(avgdl=ix.avgdl, n_docs=N_DOCS)
    return Crawl(ix, off, tok, names, copies, pages, (lone, lone_copy), z, rejected)


def site_mask(c, sites):
    """bool [N]: the pages whose URL's host equals a site or ends with "." + site (None: no restriction)."""
    if sites is None:
        return None
    hosts = [url_host(u) for u in c.ix.urls]
    return np.asarray([h is not None and any(h == s or h.endswith("." + s) for s in sites) for h in hosts], bool)


# ------------------------------------------------------------------------------------------------ the cases
@dataclass
class Batch:
    name: str
    queries: list            # the query texts
    features: list           # per query the set of FEATURES it declares
    switches: dict           # the keywords of search_batch that hold for the whole call (without mode)
    sites: list              # per query None or the sites of its `within`
    term_lists: list = None  # per query its terms (then the texts are not tokenised), or None
    lists: dict = field(default_factory=dict)                # must / must_not / must_phrases / must_not_phrases / patterns: per query
    topic: list = None       # per query the topic word whose pages its vector is near (None: a random direction)
    seeds: list = None       # per query the seed of its vector (chosen so that no two fused rows are near-tied)


def _f(*names):
    assert set(names) <= set(FEATURES)
    return set(names)


ALL_ON = dict(operators=True, proximity=True, fuzzy=True, wildcards=True, max_expansions=5, snippets=True, snippet_tokens=12,
              facets=True, facet_limit=7, collapse_duplicates=True, top_k=60, dense_k=20)
# everything on: the conditions come as lists (a quoted phrase's words and a `+word` also score, and these words stand on most
# pages: with all of them in the scoring text every BM25 sum is negative and the lexical list is empty)
_EVERYTHING = dict(must=["essen"], must_not=["geschlossen"],
                   must_phrases=[["alte", "aula"], Near(["morgens", "abends"], 1, ordered=True), Near("kuchen kaffee", 1)],
                   must_not_phrases=["kein zutritt"])


def _only_first(first, n=8):
    """The lists of a text batch: query 0 has `first`, the others nothing."""
    return {k: [list(v)] + [[] for _ in range(n - 1)] for k, v in first.items()}
_ALL12 = [f for f in FEATURES if not f.startswith("facets")]
_wf = [_word(len(NAMED) + 3 * i) for i in range(MSR_MAX_QUERY_TERMS - 1)]      # 63 known filler words


# per batch and query the seed of the query vector: the first of 7 + 1000 b + 10 q + 10000 k with which, in both modes, no two
# adjacent rows of the oracle's fused list are closer than 4e-5, no row is closer than that to diversification's relevance
# threshold 0.8, and the dense stage's last candidate leads the first page left out by 1e-4 (test_options_ref.py asserts half)
SEEDS = [[40007, 17, 27, 37, 47, 57, 10067, 77], [1007, 1017, 1027, 1037, 1047, 1057, 1067, 1077],
         [2007, 32017, 42027, 2037, 2047, 2057, 2067, 2077], [13007, 3017, 13027, 13037, 3047, 23057, 3067, 23077]]


def _batches():
    A = Batch("text, facets by host",
              ["mensaa biblio*",
               'bibliothekk "alte aula" uni*',
               'semesterticket -"kein zutritt" +essen',
               '"kuchen kaffee"~1 hochschulsportt',
               'wohnheim "morgens abends"~>1 -geschlossen',
               "t?bingen uni* mensaa bibliothekk",
               'mensa -"morgens abends"~>3 bib*',
               'bibliothek +essen "abends morgens"~2'],
              [_f(*_ALL12, "facets_host"),
               _f("fuzzy", "must_phrase", "wildcard", "facets_host", "collapse", "snippets"),
               _f("must_not_phrase", "must", "facets_host", "collapse", "snippets"),
               _f("near_unordered", "fuzzy", "facets_host", "snippets"),
               _f("near_ordered", "must_not", "within", "facets_host", "snippets"),
               _f("fuzzy", "wildcard", "facets_host", "collapse", "snippets", "within"),
               _f("near_ordered", "wildcard", "facets_host", "snippets"),
               _f("must", "near_unordered", "facets_host", "snippets")],
              dict(ALL_ON, facet_by="host"),
              [BIG_SITES, None, None, None, BIG_SITES, BIG_SITES, None, None], lists=_only_first(_EVERYTHING),
              topic=["mensa", "bibliothek", "semesterticket", None, "wohnheim", "mensa", "mensa", "bibliothek"], seeds=SEEDS[0])
    B = Batch("text, facets by domain",
              ["bibliothekk uni*",
               'mensa "alte aula" -"aula alte"',
               "semesterticket -essen",
               "uni* bib* wohnheimm",
               '+mensa +essen "kuchen kaffee"~1 -"kein zutritt"',
               'hochschulsport "morgens abends"~>1',
               'semesterticket "alte aula" -geschlossen',
               "bibliothek mensa -zutritt"],
              [_f(*_ALL12, "facets_domain"),
               _f("must_phrase", "must_not_phrase", "facets_domain", "collapse", "snippets"),
               _f("must_not", "facets_domain", "snippets", "within"),
               _f("wildcard", "fuzzy", "facets_domain", "snippets"),
               _f("must", "near_unordered", "must_not_phrase", "facets_domain", "collapse", "snippets", "within"),
               _f("near_ordered", "facets_domain", "snippets"),
               _f("must_phrase", "must_not", "facets_domain", "collapse", "snippets"),
               _f("must_not", "facets_domain", "collapse", "snippets")],
              dict(ALL_ON, facet_by="domain", facet_limit=4, snippet_tokens=30),
              [BIG_SITES, None, UNI_SITES, None, BIG_SITES, None, None, None], lists=_only_first(_EVERYTHING),
              topic=["bibliothek", "mensa", "semesterticket", None, "mensa", "hochschulsport", "semesterticket", "bibliothek"],
              seeds=SEEDS[1])
    C = Batch("lists, facets by host",
              ["mensa", "bibliothek semesterticket", "zzzzqqqq xxxxyyyy", "semesterticket", "wohnheim", "hochschulsport mensa",
               "mensa", "semesterticket bibliothek"],
              [_f("must", "must_not", "must_phrase", "facets_host", "collapse", "snippets"),
               _f("wildcard", "near_ordered", "near_unordered", "facets_host", "collapse", "snippets"),
               _f(),                                         # unknown words only
               _f("must", "collapse", "facets_host", "snippets"),             # the copy alone satisfies must=["essen"]
               _f("must"),                                   # an empty set: no page holds the second required word
               _f("within", "must_not_phrase", "facets_host", "snippets"),
               _f("fuzzy", "must", "wildcard", "facets_host", "collapse", "snippets"),
               _f("within", "must_phrase", "must_not", "facets_host", "snippets")],          # fewer than top_k pages
              dict(fuzzy=True, max_expansions=8, snippets=True, snippet_tokens=20, facets=True, facet_by="host", facet_limit=10,
                   collapse_duplicates=True, top_k=60, dense_k=20),
              [None, None, None, None, None, NET_SITES, None, UNI_SITES],
              term_lists=[["mensa"], ["bibliothek", "semesterticket"], ["zzzzqqqq", "xxxxyyyy"], ["semesterticket"], ["wohnheim"],
                          ["hochschulsport", "mensa"], ["mensa"], ["semesterticket", "bibliothek"]],
              lists=dict(must=[["essen"], [], [], ["essen"], ["essen", "zzzzqqqq"], [], ["esssen"], []],
                         must_not=[["geschlossen"], [], [], [], [], [], [], ["geschlossen"]],
                         must_phrases=[[["alte", "aula"]], [Near(["morgens", "abends"], 1, ordered=True), Near("kaffee kuchen", 1)], [],
                                       [], [], [], [], ["aula alte"]],
                         must_not_phrases=[[], [], [], [], [], [["zutritt", "kein"]], [], []],
                         patterns=[None, ["uni*"], None, None, None, None, ["Biblio*", "?", "w*"], None]),
              topic=["mensa", "bibliothek", None, "semesterticket", "wohnheim", "hochschulsport", "mensa", "semesterticket"], seeds=SEEDS[2])
    D = Batch("lists, facets by domain, mirrors only",
              ["semesterticket", " ".join(_wf) + " zzzzqqqq", "mensa", "bibliothek", "wohnheim hochschulsport", "mensa bibliothek",
               "semesterticket", "bibliothek"],
              [_f("collapse", "facets_domain", "snippets"),
               _f("facets_domain", "snippets"),              # 63 known ids, one unknown word and a pattern
               _f("near_unordered", "must_not_phrase", "facets_domain", "collapse", "snippets"),
               _f("within", "fuzzy", "facets_domain", "collapse", "snippets"),
               _f("must_not", "near_ordered", "facets_domain", "snippets"),
               _f("wildcard", "must_phrase", "facets_domain", "collapse", "snippets"),
               _f("within", "near_unordered", "facets_domain", "collapse", "snippets"),
               _f("must", "must_not_phrase", "facets_domain", "collapse", "snippets")],
              dict(fuzzy=True, max_expansions=3, snippets=True, snippet_tokens=64, facets=True, facet_by="domain", facet_limit=64,
                   collapse_duplicates=True, duplicate_threshold=1.0, top_k=60, dense_k=20),
              [None, None, None, BIG_SITES, None, None, NET_SITES + ["tuebingen.de"], None],
              term_lists=[["semesterticket"], _wf + ["zzzzqqqq"], ["mensa"], ["bibliothek", "unibibliotek"],
                          ["wohnheim", "hochschulsport"], ["mensa", "bibliothek"], ["semesterticket"], ["bibliothek"]],
              lists=dict(must=[[], [], [], [], [], [], [], ["essen"]],
                         must_not=[[], [], [], [], ["essen"], [], [], []],
                         must_phrases=[[], [], [Near(["kuchen", "kaffee"], 1)], [], [Near("abends morgens", 1, ordered=True)],
                                       [["alte", "aula"]], [Near("morgens abends", 1)], []],
                         must_not_phrases=[[], [], ["kein zutritt"], [], [], [], [], [["zutritt", "kein"]]],
                         patterns=[None, ["bib*"], None, None, None, ["*bibliothek", "uni*"], None, None]),
              topic=["semesterticket", None, "mensa", "bibliothek", "wohnheim", "mensa", "semesterticket", "bibliothek"], seeds=SEEDS[3])
    return [A, B, C, D]


BATCHES = _batches()
# beside the table: a query whose final list is longer than the 128 columns the retriever copies back per query (with the
# reranker's top_k raised to WIDE_TOP and diversification off), so that its chunk comes back in full -- with drops
WIDE_TOP = 400
WIDE = Batch("wide: more rows than the copied columns", ["mensa semesterticket", "wohnheim"], [_f(), _f()],
             dict(fuzzy=True, facets=True, facet_by="host", facet_limit=5, collapse_duplicates=True, top_k=1000, dense_k=20),
             [None, None], term_lists=[["mensa", "semesterticket"], ["wohnheim"]], topic=["mensa", "wohnheim"], seeds=[595007, 5017])
LISTS = ("must", "must_not", "must_phrases", "must_not_phrases", "patterns")


def masks(c, batch):
    return [site_mask(c, s) for s in batch.sites]


@lru_cache(maxsize=None)
def _vectors(name):
    c, batch = crawl(), next(b for b in BATCHES + [WIDE] if b.name == name)
    out = np.zeros((len(batch.queries), 768), np.float32)
    for q, w in enumerate(batch.topic or [None] * len(batch.queries)):
        out[q] = vector(c, w, batch.seeds[q])
    return out


def vector(c, topic, seed):
    """A random direction, leaning towards three of the topic's pages (the first one has copies) when there is a topic."""
    rng = np.random.default_rng(seed)
    off = np.asarray(c.ix.doc_off, np.int64)
    g = rng.standard_normal(768).astype(np.float32)
    v = g / np.linalg.norm(g)
    if topic is not None:
        for p in (c.pages[topic][0], c.pages[topic][11], c.pages[topic][30]):
            v = v + np.float32(0.2) * c.ix.emb[off[p]]
    return (v * np.float32(rng.uniform(0.5, 3.0))).astype(np.float32)


def vectors(c, batch):
    return _vectors(batch.name)


def call_kwargs(c, batch, q=None, within=None):
    """The keywords of search_batch (q=None; within: the per-query DocSet / None list the caller built from masks()) or of
    search for query q (within: that query's DocSet or None), without mode."""
    kw = dict(batch.switches)
    qv = vectors(c, batch)
    if q is None:
        kw.update(query_embeddings=qv, term_lists=batch.term_lists, within=within)
        kw.update({k: v for k, v in batch.lists.items()})
        return kw
    kw.update(query_embedding=qv[q], terms=None if batch.term_lists is None else batch.term_lists[q], within=within)
    kw.update({k: v[q] for k, v in batch.lists.items()})
    return kw
