"""Typo-tolerant search, the host's policy (DESIGN K15; the lookup itself is msr_fuzzy_terms, DeviceEngine.fuzzy_terms).

A query word the vocabulary lacks is replaced by the nearest vocabulary term: distance = optimal string alignment over code
points (insertion, deletion, substitution, swap of two adjacent code points), nearest = smallest distance, then largest
document frequency, then smallest term id.  How far a word may be from its replacement is auto_edits(length): the widely
used AUTO rule.  Only words that came out of the tokenizer and that CorpusIndex.term_ids mapped to -1 are looked up; words of
the vocabulary are never touched; required words (must= / `+word`) are corrected the same way.  Excluded words (must_not= /
`-word`), phrases and proximity conditions are NOT corrected: excluding or quoting a guessed word is wrong more often than
right.  Pure Python: nothing here needs a GPU.
"""
import re

import numpy as np

MSR_FUZZY_MAX_LEN = 32        # code points of the longest word that is looked up and of the longest term that is suggested
MAX_CODE_POINT = 0xFFFE       # a word or term holding a code point above it is left alone (the device compares 16-bit units)


def auto_edits(n_codepoints):
    """The AUTO rule: 0 edits below 3 code points, 1 for 3 .. 5, 2 from 6 up."""
    n = int(n_codepoints)
    return 0 if n < 3 else 1 if n < 6 else 2


def lookable(word):
    """True if `word` can be looked up (and, for a term, suggested): a string of 1 .. MSR_FUZZY_MAX_LEN code points, none
    above MAX_CODE_POINT."""
    return isinstance(word, str) and 1 <= len(word) <= MSR_FUZZY_MAX_LEN and max(map(ord, word)) <= MAX_CODE_POINT


def encode_words(words):
    """-> (word_off int32 [n + 1], word_chars uint16) of lookable words, as msr_fuzzy_terms reads them."""
    off = np.zeros(len(words) + 1, np.int32)
    if words:
        np.cumsum([len(w) for w in words], out=off[1:])
    return off, np.asarray([ord(c) for w in words for c in w], np.uint16)


def vocab_image(vocab, term_off):
    """-> (char_off int64 [V + 1], chars uint16, weight uint32 [V]) of a vocabulary {term: id} with postings offsets term_off:
    term id t's code points and its document frequency term_off[t + 1] - term_off[t] -- 0, so that it is never suggested, for
    a term that is not lookable() and for an id no term of `vocab` names (its code points are then empty)."""
    V = int(len(term_off)) - 1
    names = [""] * V
    for s, t in vocab.items():
        if 0 <= int(t) < V and lookable(s):
            names[int(t)] = s
    weight = np.diff(np.asarray(term_off, np.int64)).astype(np.int64)
    if V and int(weight.max(initial=0)) >= 2 ** 31:
        raise ValueError("vocab_image: a document frequency of 2^31 or more")
    weight = np.where(np.asarray([bool(s) for s in names], bool), weight, 0).astype(np.uint32) if V else np.zeros(0, np.uint32)
    char_off = np.zeros(V + 1, np.int64)
    if V:
        np.cumsum([len(s) for s in names], out=char_off[1:])
    return char_off, np.asarray([ord(c) for s in names for c in s], np.uint16), weight


def unknown_words(term_lists, id_lists):
    """The words to look up, each once, in first-occurrence order: strings whose id is -1 and that are lookable() with a
    tolerance above 0.  term_lists / id_lists: parallel lists (per query) of terms and of their ids (CorpusIndex.term_ids)."""
    seen = {}
    for terms, ids in zip(term_lists, id_lists):
        for t, i in zip(terms, ids):
            if int(i) < 0 and t not in seen and lookable(t) and auto_edits(len(t)) > 0:
                seen[t] = None
    return list(seen)


def correct(lookup, name_of, terms, ids, must=None, must_ids=None):
    """The replacement policy for a chunk of queries.  terms / ids: per query its scoring terms and their ids; must / must_ids:
    the same for the required terms (None: none).  lookup(words) -> per word the id of its first candidate or -1 -- called
    ONCE, with every unknown word of the chunk, and not at all when there is none.  name_of(term id) -> the term string.
    -> (ids, must_ids, corrections): new id lists in which a -1 that had a candidate holds that candidate's id, everything
    else as it was, and per query {typed term: used term} (empty: nothing replaced).  The inputs are not modified; excluded
    terms and phrases are not arguments on purpose: they are never corrected."""
    Q = len(terms)
    both_t = [list(terms[q]) + (list(must[q]) if must is not None else []) for q in range(Q)]
    both_i = [list(ids[q]) + (list(must_ids[q]) if must_ids is not None else []) for q in range(Q)]
    words = unknown_words(both_t, both_i)
    found = {}
    if words:
        found = {w: int(t) for w, t in zip(words, lookup(words)) if int(t) >= 0}
    corrections = [{} for _ in range(Q)]

    def fix(q, ts, is_):
        out = []
        for t, i in zip(ts, is_):
            if int(i) < 0 and isinstance(t, str) and t in found:
                i = found[t]
                corrections[q][t] = name_of(i)
            out.append(i)
        return out
    new_ids = [fix(q, terms[q], ids[q]) for q in range(Q)]
    new_must = None if must_ids is None else [fix(q, must[q], must_ids[q]) if must is not None else list(must_ids[q])
                                              for q in range(Q)]
    return new_ids, new_must, corrections


_WORD = re.compile(r"\w+", re.UNICODE)


def corrected_text(processed_query, corrections):
    """The processed query with every typed term replaced by the term that was used, or None when nothing was replaced."""
    if not corrections:
        return None
    return _WORD.sub(lambda m: corrections.get(m.group(0).lower(), m.group(0)), processed_query)


class Results(list):
    """A result list that also says what was corrected: `corrections` {typed term: used term} (empty: nothing) and
    `corrected_query` (the processed query with the replacements, or None) -- and, with wildcards=True (DESIGN K16), what its
    patterns were expanded to: `expansions` {pattern: {"terms": [...], "total": n, ...}} (wildcard.expand; empty: no
    pattern) -- and, with facets=True (DESIGN K17), what the whole match set holds: `hits` (pages that match at all, None
    without facets), `facets` ([{"value": name, "count": n}, ...], the values with the most matching pages first) and
    `facet_values` (the number of distinct values hit) -- and, with collapse_duplicates=True (DESIGN K18), `collapsed`: the
    number of near-duplicate rows dropped from the list (the rows that swallowed them carry "duplicates") -- and, with match=
    (DESIGN K19), `match`: {"slots": [[term, ...], ...], "need": m}, the query's slots and how many of them every row's page
    fills (None without match=).  Equal to the plain list of its rows."""
    corrections = {}
    corrected_query = None
    expansions = {}
    hits = None
    facets = []
    facet_values = 0
    collapsed = 0
    match = None

    def __init__(self, rows=(), corrections=None, corrected_query=None, expansions=None, hits=None, facets=None,
                 facet_values=0, collapsed=0, match=None):
        super().__init__(rows)
        self.corrections = dict(corrections or {})
        self.corrected_query = corrected_query
        self.expansions = dict(expansions or {})
        self.hits = None if hits is None else int(hits)
        self.facets = list(facets or [])
        self.facet_values = int(facet_values)
        self.collapsed = int(collapsed)
        self.match = match
