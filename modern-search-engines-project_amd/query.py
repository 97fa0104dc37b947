"""A query's options and conditions as two values, and the one place that applies the text syntax.

    opts = SearchOptions(operators=True, wildcards=True)           # the switches and limits of a call
    explicit = Conditions(must=[["mensa"], []])                   # the per-query lists a caller passes beside the text
    scoring, embed, cond, patterns = parse_queries(texts, tokenize, opts, explicit, None)

Retriever (search / search_batch / batch_search, after preprocess_query) and BM25.search go through parse_queries; what the
conditions and patterns then cost on the device is theirs.  Pure Python: nothing here needs a GPU.
"""
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import facets as _facets
from ._abi import MSR_PROX_MAX_SPAN, MSR_SIG_WORDS, MSR_WILD_MAX_LIMIT
from .text import Near, parse_operators, parse_phrases, parse_proximity
from .wildcard import parse_wildcards

MODES = ("lexical", "hybrid")


@dataclass(frozen=True)
class SearchOptions:
    """The switches and limits of a search call -- the keywords of the same names of Retriever.search / search_batch /
    batch_search and BM25.search.  Everything is off by default, and without a feature the call uploads, launches and returns
    exactly what it did before the feature existed.  Where the index or the engine lacks what a feature needs, the facade
    that holds them raises before any device work (Retriever._check_options, BM25.search).

    mode="hybrid": the dense top dense_k documents join the BM25 candidates (a page that shares no term with the query can
    be returned; a query of unknown words only still gets results); every row then carries "matched_by": "lexical" |
    "dense" | "both".  mode="lexical" (default): the reference's path, rows without that key.
    operators=True: `+word` / `-word` tokens of a query (text.parse_operators, after preprocess_query) name words every
    result must / must not contain; `+word` still scores, `-word` does not.  must / must_not (Conditions): per query a list
    of term strings (for callers with their own tokenizer, like term_lists), joined with the parsed ones.  Both act inside
    `within`, in both stages of either mode: a page that holds an excluded word is never returned.
    phrases=True: `"a b c"` in a query is a required phrase (its words still score), `-"a b"` an excluded one (removed from
    the scoring text) -- text.parse_phrases, after preprocess_query and before the operators; must_phrases /
    must_not_phrases (Conditions): per query a list of phrases, each a string (tokenised like the query) or a list of term
    strings.  A result holds every required phrase and no excluded one IN ITS INDEXED TOKEN STREAM (words next to each other,
    in order, after the tokenizer); the scores are unchanged.  Needs an index with a forward index
    (index_build.attach_tokens; MsrError otherwise); a phrase of more than 16 terms raises ValueError.
    proximity=True: phrases=True, and `"a b"~N` / `"a b"~>N` are proximity conditions (text.parse_proximity): the words
    within a window with up to N other tokens among them, in any order / in this order.  A text.Near in must_phrases /
    must_not_phrases (terms: a string or a list of term strings) is such a condition without the text syntax.  A slop
    below 0, more than 16 terms or a window of more than 64 tokens raises ValueError.
    snippets=True (DESIGN K14): every row's "snippet" is the passage of the page that holds the most of the query -- the
    window of snippet_tokens (1 .. 64) tokens of its indexed stream with the largest summed weight of distinct query terms
    (snippets.term_weights: the idf; then the most occurrences, then the earliest), found by ONE DeviceEngine.best_windows
    call for all returned documents of the call and cut from the page by snippets.render -- and the row gains
    "highlights" ([begin, end) offsets of the query's terms in the snippet) and "missing" (the query's terms the passage
    lacks).  Documents, ranks and scores are unchanged.  A page without a query term (a dense-only hybrid hit) and a
    query of unknown words keep the reference's snippet, with "highlights": [] and every term of the row missing.  A
    custom tokenizer needs Retriever(span_tokenizer=...) (ValueError); the index needs a forward index and texts (MsrError).
    fuzzy=True (DESIGN K15): a query word the vocabulary lacks -- otherwise silently dropped -- is replaced by its nearest
    vocabulary term before stage 1: optimal string alignment distance (insertion, deletion, substitution, swap of two
    adjacent code points) within the AUTO tolerance of the word's length (0 edits below 3 code points, 1 for 3 .. 5, 2
    from 6 up), then the largest document frequency, then the smallest term id; ONE DeviceEngine.fuzzy_terms call per
    chunk of queries.  Words of the vocabulary are never touched; must= / `+word` terms are corrected the same way;
    must_not / `-word` terms, phrases and proximity conditions are NOT (excluding or quoting a guessed word is wrong more
    often than right).  Correction is lexical: the dense stage and the reranker use the embedding of the query AS TYPED.
    Each query's result is then a fuzzy.Results list -- the same rows, plus `corrections` ({typed term: used term}, empty if
    none) and `corrected_query` (the processed query with the replacements, or None).  Needs an index with term strings
    (ValueError).
    wildcards=True (DESIGN K16): a query token with `*` (any run of code points) or `?` (exactly one) -- `bibliothek*`,
    `*bibliothek`, `t?bingen` -- is a pattern (wildcard.parse_wildcards: only letters and the two metacharacters, one
    trailing `?` is punctuation, nothing inside quotes): it leaves the scoring text, and the vocabulary terms it matches as
    a whole, the most frequent first, at most max_expansions (1 .. 16) of them, are appended to the query's terms as
    ordinary scoring terms (wildcard.expand: no id twice, at most MSR_MAX_QUERY_TERMS unique ids, a pattern with fewer
    than two literal code points is skipped; a word the vocabulary lacks and fuzzy=True did not replace still takes ONE of
    those MSR_MAX_QUERY_TERMS places -- the engine packs it as a term of its own and refuses a query of more); ONE
    DeviceEngine.wildcard_terms call per chunk of queries.  patterns=: per query a list of further pattern strings, with
    or without wildcards=True.  Patterns match the vocabulary AS INDEXED
    (lemmas, with a lemmatising tokenizer); they are never required, excluded (`+uni*` / `-uni*`: ValueError), part of a
    phrase, or corrected by fuzzy=True; hybrid mode scores the expanded terms in its lexical half and the dense stage keeps
    the embedding of the query as typed.  Each query's result is then a fuzzy.Results list whose `expansions` maps each
    pattern to {"terms": the terms used, "total": all matches, "skipped" / "truncated": True where that happened}.  Needs
    an index with term strings; max_expansions outside 1 .. 16 raises ValueError.
    facets=True (DESIGN K17): each query's result is a fuzzy.Results list that also says what the WHOLE match set holds,
    counted on the device (ONE DeviceEngine.facet_counts call per chunk of queries), not over the ~100 rows returned:
    `hits` -- the pages that hold at least one counting term of the query (facets.counting_terms: the scored terms with
    idf > 0, so not the city term preprocessing appends; all of them if none has) inside within= and inside what
    operators, phrases and proximity built; it is NOT the length of BM25's unlimited list under an arbitrary min_score --
    `facets` -- [{"value": name, "count": pages}, ...], the first facet_limit (1 .. 64, ValueError otherwise) values by
    (count desc, first occurrence in the index asc) -- and `facet_values`, the number of distinct values hit.  facet_by:
    "host" (default: docset.url_host, so a value can be handed back as a site of DocSet.from_sites / sites=[...]) or
    "domain" (the rows' "domain" key); anything else raises ValueError.  The terms counted are the ones scored: after
    fuzzy correction and wildcard expansion.  mode="hybrid" counts the LEXICAL matches only (a dense-only hit is in no
    count).  A query of unknown words has 0 hits and no facets.  The table of facet_by is bound lazily per index and again
    after update_index.  An index without URLs raises ValueError.
    collapse_duplicates=True (DESIGN K18): pages that differ in URL and not in content -- `www.` against the bare host,
    `http` against `https`, print views, mirrors -- are shown once.  Every document has a min-hash signature of 64 words over
    the 4-token shingles of its indexed stream (ONE DeviceEngine.doc_signatures call per index, bound lazily and again after
    update_index); between fuse and diversification ONE DeviceEngine.collapse_duplicates call per chunk of queries walks each
    fused list in rank order and drops a row whose signature agrees with an earlier KEPT row's in at least
    ceil(duplicate_threshold * 64) words (the share of equal words estimates the Jaccard overlap of the two pages' shingle
    sets; duplicate_threshold in (0, 1], ValueError otherwise; default 0.9 -> 58 of 64).  A dropped row leads nothing: of
    A ~ B ~ C with A unlike C, A and C stay.  A page the response models reject and a page without tokens neither drop nor
    lead.  Each query's result is then a fuzzy.Results list whose `collapsed` is the number of rows dropped, and every row
    that swallowed one gains "duplicates": [{"doc_id", "url", "title", "similarity": equal words / 64}, ...] in the order
    they were dropped; rows that swallowed nothing lack the key.  The scores are unchanged, diversification then works on
    the collapsed list, matched_by and snippets are those of the rows that stay, and facets=True still counts ALL matches,
    copies included.  Needs an index with a forward index (MsrError).
    match="all" | m | "75%" (DESIGN K19; default "any": every search is an OR and ranking alone decides): a result must hold
    ALL of the query's words, or at least m of them.  The words are the query's slots (match.slots): every distinct scored
    word with idf > 0 is a slot (so the city term that preprocessing appends is none, and neither is a typed `tübingen`), a
    word the vocabulary lacks is a slot that no page fills (match="all" then returns nothing, as `+word` does; fuzzy=True runs
    first and may have replaced it), and the expansions of one wildcard pattern are ONE slot that any of them fills.  How
    many slots a page must fill is match.need: "all" -- all G; an int m -- m, a negative one all but |m|; "75%" -- floor(0.75
    G), "-25%" -- G less floor(0.25 G); always at least 1 and at most G (Lucene's minimum_should_match rule).  A bool, 0,
    "0%", a float or another string raises ValueError.  ONE match.match_sets call per chunk of queries counts the slots on
    the device, inside within= and inside what operators, phrases and proximity built, and its rows restrict BOTH stages of
    either mode: a result of match="all" holds all the words whichever stage found it.  Scores and the order among the pages
    that stay are unchanged.  Each query's result is then a fuzzy.Results list whose `match` is {"slots": [[term, ...],
    ...], "need": m} (need None: the query has no slot, nothing was restricted).  With facets=True `hits` and `facets` count
    inside the matched set -- "how many pages hold all my words" -- because they count inside the restriction."""
    mode: str = "lexical"
    dense_k: int = 100
    operators: bool = False
    phrases: bool = False
    proximity: bool = False
    snippets: bool = False
    snippet_tokens: int = 30
    fuzzy: bool = False
    wildcards: bool = False
    max_expansions: int = 8
    facets: bool = False
    facet_by: str = "host"
    facet_limit: int = 10
    collapse_duplicates: bool = False
    duplicate_threshold: float = 0.9
    match: object = "any"

    @property
    def min_matches(self):
        """Equal signature words (of MSR_SIG_WORDS) from which two pages are duplicates: ceil(duplicate_threshold * 64)."""
        return int(math.ceil(float(self.duplicate_threshold) * MSR_SIG_WORDS))

    @property
    def match_on(self):
        """True unless match is "any" or None: only then is match.py imported and anything of it uploaded or launched."""
        return not (self.match is None or (isinstance(self.match, str) and self.match == "any"))

    def check(self, patterns=False, int_types=(int, np.integer)):
        """ValueError unless the values are in range: the mode; the match value (match.check_value); and of the features that are on, snippet_tokens of 1 ..
        MSR_PROX_MAX_SPAN, the facet key and limit (facets.check_options), max_expansions of 1 .. MSR_WILD_MAX_LIMIT
        (patterns: the call has explicit patterns, which need it like wildcards=True), duplicate_threshold in (0, 1].  int_types: what counts as a whole
        number (BM25.search takes no numpy integer)."""
        whole = lambda v, top: not isinstance(v, bool) and isinstance(v, int_types) and 1 <= int(v) <= top
        if self.mode not in MODES:
            raise ValueError(f"mode must be 'lexical' or 'hybrid' (got {self.mode!r})")
        if self.snippets and not whole(self.snippet_tokens, MSR_PROX_MAX_SPAN):
            raise ValueError(f"snippet_tokens must be 1 .. MSR_PROX_MAX_SPAN = {MSR_PROX_MAX_SPAN} (got {self.snippet_tokens!r})")
        if self.facets:
            _facets.check_options(self.facet_by, self.facet_limit)
        if (self.wildcards or patterns) and not whole(self.max_expansions, MSR_WILD_MAX_LIMIT):
            raise ValueError(f"max_expansions must be 1 .. MSR_WILD_MAX_LIMIT = {MSR_WILD_MAX_LIMIT} (got {self.max_expansions!r})")
        if self.collapse_duplicates:
            t = self.duplicate_threshold
            if isinstance(t, bool) or not isinstance(t, (int, float, np.integer, np.floating)) or not 0.0 < float(t) <= 1.0:
                raise ValueError(f"duplicate_threshold must be in (0, 1] (got {t!r})")
        if self.match_on:
            from .match import check_value
            check_value(self.match)


@dataclass(frozen=True)
class Conditions:
    """What the results of each query must and must not hold: must / must_not (per query a list of terms), must_phrases /
    must_not_phrases (per query a list of phrases: a list of terms, a string still to be tokenised, or a text.Near), each None
    or a list of one entry per query.  The pair rule: where no query has a term of either kind must and must_not are BOTH
    None, and so are the phrase lists -- the chain then launches exactly what it does without the feature."""
    must: Optional[list] = None
    must_not: Optional[list] = None
    must_phrases: Optional[list] = None
    must_not_phrases: Optional[list] = None

    def _lists(self):
        return (("must", self.must), ("must_not", self.must_not), ("must_phrases", self.must_phrases),
                ("must_not_phrases", self.must_not_phrases))

    @property
    def empty(self):
        return all(lists is None for _, lists in self._lists())

    def check(self, Q):
        """ValueError unless every list that is given has Q entries."""
        for name, lists in self._lists():
            if lists is not None and len(lists) != Q:
                raise ValueError(f"{name}: {len(lists)} entries for {Q} queries")

    def slice(self, a, b):
        """The conditions of queries a .. b."""
        return Conditions(*(None if lists is None else lists[a:b] for _, lists in self._lists()))

    def ids(self, term_ids, tokenize):
        """The same conditions over term ids (term_ids: CorpusIndex.term_ids).  A phrase is a list of terms here; a text.Near
        keeps its slop and mode, and its terms may still be a string (tokenised like the query)."""
        def phrase(p):
            if isinstance(p, Near):
                return p.with_terms(term_ids(tokenize(p.terms) if isinstance(p.terms, str) else list(p.terms)))
            return term_ids(p)
        terms = lambda lists: None if lists is None else [term_ids(t) for t in lists]
        phrases = lambda lists: None if lists is None else [[phrase(p) for p in ps] for ps in lists]
        return Conditions(terms(self.must), terms(self.must_not), phrases(self.must_phrases), phrases(self.must_not_phrases))

    def sets(self, engine, within):
        """Conditions over term ids -> what takes within's place: the DeviceSets of ONE DeviceEngine.phrase_sets call when a
        phrase list is given, else of ONE term_sets call when a term list is, else `within` itself."""
        if self.must_phrases is not None or self.must_not_phrases is not None:
            return engine.phrase_sets(self.must_phrases, self.must_not_phrases, self.must, self.must_not, within=within)
        if self.must is not None or self.must_not is not None:
            return engine.term_sets(self.must, self.must_not, within=within)
        return within


def parse_queries(texts, tokenize, opts, explicit=Conditions(), patterns=None, drop_empty=False):
    """The text syntax of SearchOptions, applied to every query -> (scoring texts, texts to embed or None, Conditions,
    patterns).  In this order: wildcards (wildcard.parse_wildcards, on the text that still has its quotes), then proximity
    or phrases, then operators; then each query's explicit conditions (`explicit`) and, behind them, the parsed ones, the
    words and phrases tokenised like the query, are joined and a phrase that tokenises to nothing is dropped.
    texts: the queries, ready to be parsed (Retriever: after preprocess_query).  patterns: None or per query None / a list
    of pattern strings (ValueError for anything else), lower-cased here, behind the parsed ones; the patterns come back as
    a list per query when wildcards is on or `patterns` is given, else None.
    The text to embed differs from the scoring text where a pattern was taken out: it keeps the pattern (the dense stage
    sees the query as typed), operators and phrases are still taken out of it; None when no text lost a pattern.
    drop_empty (BM25.search, which returns [] for such a query before it looks at its conditions): a query whose scoring
    text has no token and that has no pattern gets no conditions."""
    Q = len(texts)
    scoring, embed, pats = list(texts), None, None
    if opts.wildcards or patterns is not None:
        pats = [[] for _ in range(Q)]
        if opts.wildcards:
            for q, (text, found) in enumerate(map(parse_wildcards, texts)):
                scoring[q], pats[q] = text, list(found)
        if patterns is not None:
            if len(patterns) != Q:
                raise ValueError(f"patterns: {len(patterns)} entries for {Q} queries")
            for q, ps in enumerate(patterns):
                if isinstance(ps, str) or not all(isinstance(p, str) for p in (ps or ())):
                    raise ValueError("patterns: per query a LIST of pattern strings")
                pats[q] += [p.lower() for p in (ps or ())]
    quoted = parse_proximity if opts.proximity else parse_phrases if opts.phrases else None
    if quoted is None and not opts.operators and explicit.empty:
        return scoring, (None if scoring == list(texts) else list(texts)), explicit, pats
    explicit.check(Q)

    def strip(text):
        """-> (text, required phrases, excluded phrases, required words, excluded words)"""
        m_ph, x_ph, m_words, x_words = [], [], [], []
        if quoted is not None:
            text, m_ph, x_ph = quoted(text)
        if opts.operators:
            text, m_words, x_words = parse_operators(text)
        return text, m_ph, x_ph, m_words, x_words
    if scoring != list(texts):
        embed = [strip(t)[0] for t in texts]
    as_terms = lambda p: (p.with_terms(as_terms(p.terms)) if isinstance(p, Near) else tokenize(p) if isinstance(p, str) else list(p))
    given = lambda lists, q: [] if lists is None else list(lists[q])
    m, x, mp, xp = ([[] for _ in range(Q)] for _ in range(4))
    for q in range(Q):
        scoring[q], m_ph, x_ph, m_words, x_words = strip(scoring[q])
        if drop_empty and not (pats and pats[q]) and not tokenize(scoring[q]):
            continue
        m[q] = given(explicit.must, q) + [t for w in m_words for t in tokenize(w)]
        x[q] = given(explicit.must_not, q) + [t for w in x_words for t in tokenize(w)]
        mp[q] = [p for p in map(as_terms, given(explicit.must_phrases, q) + m_ph) if p]
        xp[q] = [p for p in map(as_terms, given(explicit.must_not_phrases, q) + x_ph) if p]
    if not any(m) and not any(x):
        m = x = None
    if not any(mp) and not any(xp):
        mp = xp = None
    return scoring, embed, Conditions(m, x, mp, xp), pats
