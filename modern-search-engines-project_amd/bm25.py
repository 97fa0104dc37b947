"""BM25 facade with the reference's signature and return shape (indexer/bm25_indexer.py:57,383-514).

    BM25(index_or_engine, k1=1.2, b=0.75).search(query, top_k=1000, min_score=0.0)
        -> [{"doc_id": int, "score": float, "text_snippet": str}, ...]

The reference opens a DuckDB file and re-reads postings per query; here the postings are already in HBM
(DeviceEngine) and the scoring loop + sort + cut run as msr_bm25_topk.  The host keeps what is host work
in the reference too: tokenising the query string and formatting the snippet.
"""
from dataclasses import replace
from typing import Callable, List, Optional, Sequence, Union

from . import fuzzy as _fuzzy
from . import wildcard as _wildcard
from .engine import DeviceEngine
from .index import CorpusIndex
from .query import Conditions, SearchOptions, parse_queries
from .serial import serialised
from .text import simple_tokenize


class BM25:
    def __init__(self, source: Union[CorpusIndex, DeviceEngine], k1: float = 1.2, b: float = 0.75,
                 tokenizer: Optional[Callable[[str], List[str]]] = None, device=0, **engine_kw):
        if isinstance(source, DeviceEngine):
            self.engine = source
        else:
            source.k1, source.b = k1, b
            self.engine = DeviceEngine(source, device=device, **engine_kw)
        self._tokenize = tokenizer or simple_tokenize
        self.attach(self.engine.index)

    @serialised
    def attach(self, index: CorpusIndex):
        """Point the facade at the index its engine now serves (DeviceEngine.rebind)."""
        self.index = index
        self.k1, self.b = index.k1, index.b
        self._pos = None
        self._names = None

    def _name_of(self, t):
        if self._names is None:
            self._names = {v: k for k, v in (self.index.vocab or {}).items()}
        return self._names.get(int(t), str(t))

    def _check_fuzzy(self):
        if not self.engine.has_vocab:
            raise ValueError("fuzzy: the index has no vocabulary (CorpusIndex.vocab: term strings); a term-id-only index cannot "
                             "correct a word")

    def _lookup(self, words):
        """fuzzy.correct's lookup: per word the id of its first candidate or -1 (ONE DeviceEngine.fuzzy_terms call)."""
        return [c[0][0] if c else -1 for c, _ in self.engine.fuzzy_terms(words, limit=1)]

    @serialised
    def fuzzy_terms(self, words, limit=5):
        """Which vocabulary words are near these?  -> per word a list of (term, distance, doc_freq), nearest first (distance,
        then document frequency descending), at most `limit` of them, within the AUTO tolerance of the word's length (0 edits
        below 3 code points, 1 for 3 .. 5, 2 from 6 up); a word of the vocabulary comes first in its own list, at distance
        0.  One DeviceEngine.fuzzy_terms call (msr_fuzzy_terms, DESIGN K15)."""
        import numpy as np
        from .index import _np
        self._check_fuzzy()
        df = np.diff(_np(self.index.term_off).astype(np.int64))
        return [[(self._name_of(t), d, int(df[t])) for t, d in cands] for cands, _ in self.engine.fuzzy_terms(list(words), limit=limit)]

    @serialised
    def wildcard_terms(self, patterns, limit=8):
        """Which vocabulary words does each pattern match (`*` any run of code points, `?` exactly one, anchored at both
        ends)?  -> per pattern ([(term, doc_freq), ...], total): the most frequent first (then the smaller term id), at most
        `limit` (1 .. 16) of them, and the number of all matches.  Patterns are lower-cased like a query.  One
        DeviceEngine.wildcard_terms call (msr_wildcard_terms, DESIGN K16); an index without term strings raises ValueError."""
        import numpy as np
        from .index import _np
        if not self.engine.has_vocab:
            raise ValueError("wildcards: the index has no vocabulary (CorpusIndex.vocab: term strings); a term-id-only index "
                             "cannot expand a pattern")
        df = np.diff(_np(self.index.term_off).astype(np.int64))
        got = self.engine.wildcard_terms([str(p).lower() for p in patterns], limit=limit)
        return [([(self._name_of(t), int(df[t])) for t in terms], total) for terms, total in got]

    # -- engine-level entry points (usable without spaCy: pre-tokenised terms or term ids) ----------
    @serialised
    def search_terms(self, terms: Sequence[Union[str, int]], top_k: int = 1000, min_score: float = 0.0, within=None):
        return self.search_terms_batch([terms], top_k, min_score, within=within)[0]

    @serialised
    def search_terms_batch(self, term_lists, top_k: int = 1000, min_score: float = 0.0, within=None):
        """-> per query: list of (doc_id, score) in rank order (before the urlsDB join).  within: None, a DocSet (every query)
        or a list of DocSet / None per query -- the top_k of the documents in the set (docset.py)."""
        ids = [self.index.term_ids(t) for t in term_lists]
        doc, score, n = self.engine.bm25_topk(ids, k=top_k, min_score=min_score, within=within)
        doc, score, n = doc.cpu().numpy(), score.cpu().numpy(), n.cpu().numpy()
        doc_ids = self.index.doc_ids
        doc_ids = doc_ids.cpu().numpy() if hasattr(doc_ids, "cpu") else doc_ids
        return [[(int(doc_ids[d]), float(s)) for d, s in zip(doc[q, :n[q]], score[q, :n[q]])] for q in range(len(ids))]

    # -- BM25 scores of named documents (msr_bm25_score_docs) -----------------------------------------
    @serialised
    def score_terms(self, terms: Sequence[Union[str, int]], doc_ids):
        """-> [(doc_id, score, matched)] in the order of doc_ids: the BM25 score search_terms gives (query, document) -- also
        for documents outside its top_k or below its min_score -- and whether the document holds any of the terms (False:
        score 0.0).  What a caller of POST /rerank needs who has doc ids but no similarities.  A doc_id the index does not
        hold raises KeyError."""
        import numpy as np
        ids = np.asarray([int(d) for d in doc_ids], np.int64).reshape(-1)
        have = self.index.doc_ids
        have = np.asarray(have.cpu().numpy() if hasattr(have, "cpu") else have, np.int64)
        if len(ids) == 0:
            return []
        pos = np.minimum(np.searchsorted(have, ids), max(len(have) - 1, 0))
        bad = ids[have[pos] != ids] if len(have) else ids
        if len(bad):
            raise KeyError(f"doc_id {int(bad[0])} is not in the index")
        score, touched = self.engine.bm25_score_docs([self.index.term_ids(terms)], pos.astype(np.int32).reshape(1, -1))
        score, touched = score.cpu().numpy()[0], touched.cpu().numpy()[0]
        return [(int(d), float(s), bool(t)) for d, s, t in zip(ids, score, touched)]

    @serialised
    def score_docs(self, query: str, doc_ids):
        """score_terms for a query string (tokenised like search)."""
        return self.score_terms(self._tokenize(query), doc_ids)

    # -- the reference's method ------------------------------------------------------------------------
    @serialised
    def search(self, query: str, top_k: int = 1000, min_score: float = 0.0, within=None, operators: bool = False,
               must=None, must_not=None, phrases: bool = False, must_phrases=None, must_not_phrases=None,
               proximity: bool = False, fuzzy: bool = False, wildcards: bool = False, max_expansions: int = 8, patterns=None,
               match="any"):
        """The switches and lists are query.SearchOptions' and query.Conditions', for this ONE query: must / must_not are one
        list of term strings (or ids) each, must_phrases / must_not_phrases one list of phrases (strings, lists of term
        strings or ids, text.Near), patterns one list of pattern strings.  The query is taken as it is -- no city is appended
        here.  The conditions restrict the documents on the device (DeviceEngine.term_sets / phrase_sets), inside `within`;
        with fuzzy=True or patterns the result is a fuzzy.Results list (`corrections`, `corrected_query`, `expansions`).
        match ("all", m, "75%": SearchOptions): only pages that fill enough of the query's slots (match.slots -- no city
        term is appended here, so every word with idf > 0 is one), counted on the device by ONE match.match_sets call; the
        result is then a fuzzy.Results list with `match`."""
        opts = SearchOptions(operators=operators, phrases=phrases, proximity=proximity, fuzzy=fuzzy, wildcards=wildcards,
                             max_expansions=max_expansions, match=match)
        one = lambda v: None if v is None else [v]
        explicit = Conditions(one(must), one(must_not), one(must_phrases), one(must_not_phrases))
        opts.check(patterns=patterns is not None, int_types=int)
        if (wildcards or patterns is not None) and not self.engine.has_vocab:
            raise ValueError("wildcards: the index has no vocabulary (CorpusIndex.vocab: term strings); a term-id-only "
                             "index cannot expand a pattern")
        (query,), _, cond, pats = parse_queries([query], self._tokenize, opts, explicit,       # (a pattern goes through str())
                                                None if patterns is None else [[str(p) for p in patterns]], drop_empty=True)
        pats = None if pats is None else pats[0]
        query_terms = self._tokenize(query)
        if not query_terms and not pats:
            return []                                              # bm25_indexer.py:396-397
        m = [] if cond.must is None else cond.must[0]
        ids = self.index.term_ids
        corrections = None
        words = list(query_terms)
        if fuzzy:
            self._check_fuzzy()
            new_ids, new_must, corr = _fuzzy.correct(self._lookup, self._name_of, [query_terms], [ids(query_terms)], [m], [ids(m)])
            query_terms, m, corrections = new_ids[0], new_must[0], corr[0]
        if not cond.empty:
            c = replace(cond, must=None if cond.must is None else [m]).ids(ids, self._tokenize)
            within = c.sets(self.engine, None if within is None else [within])
        expansions = None
        typed = query_terms
        if pats is not None:
            new_ids, exp = _wildcard.expand(lambda ps: self.engine.wildcard_terms(ps, limit=max_expansions), self._name_of,
                                            [ids(query_terms)], [pats], max_expansions)
            query_terms, expansions = new_ids[0], exp[0]
        info = None
        if opts.match_on:                                          # on top of the conditions' sets, in front of the scoring
            from . import match as _match
            typed_ids = ids(typed)
            groups = _match.slots(self.index, typed_ids,
                                  None if expansions is None else [ids(e["terms"]) for e in expansions.values()])
            n = _match.need(match, len(groups))
            unknown = [w for w, t in zip(words, typed_ids) if not 0 <= int(t) < self.index.n_terms]
            info = {"slots": _match.slot_names(groups, self._name_of, unknown), "need": n}
            if n is not None:
                within = _match.match_sets(self.engine, [groups], [n], within)
        rows = self._finish(self.search_terms(query_terms, top_k, min_score, within=within))
        if corrections is None and expansions is None and info is None:
            return rows
        return _fuzzy.Results(rows, corrections, _fuzzy.corrected_text(query, corrections) if corrections else None, expansions,
                              match=info)

    def _finish(self, ranked):
        """urlsDB join after the cut: documents without a row are dropped, snippet = title + 200 chars
        (bm25_indexer.py:490-512)."""
        ix = self.index
        if ix.urls is None:
            return [{"doc_id": d, "score": s, "text_snippet": None} for d, s in ranked]
        pos = getattr(self, "_pos", None)
        if pos is None:
            ids = ix.doc_ids.cpu().numpy() if hasattr(ix.doc_ids, "cpu") else ix.doc_ids
            pos = self._pos = {int(d): i for i, d in enumerate(ids)}
        out = []
        for d, s in ranked:
            i = pos[d]
            if ix.urls[i] is None:                                 # no urlsDB row
                continue
            title, text = ix.titles[i], ix.texts[i]
            snip = f"{title or 'N/A'}: {text[:200]}"
            if len(text or "") > 200:
                snip += "..."
            out.append({"doc_id": d, "score": s, "text_snippet": snip})
        return out
