"""Shared cases and the plain Python reference of query-biased snippets (msr_best_windows, DESIGN K14).

    best_window(stream, terms, weights, span, n_terms) -> (start, cover, hits, mask, terms)   the definition of msretr.h: plain
                                                                                              loops over every start
    best_window_2(...)                                                                        the same by other means: one
                                                                                              sliding window with a count per id
    best_windows_fast(tok_off, tok_ids, pair_doc, pair_row, rows, weights, spans, n_terms)    the same over a forward index at
                                                                                              once (numpy prefix sums)
    hand() -> SnipCorpus            hand-made streams: chunk geometry, document ends, neighbours, every kind of row
    corpus_cases(N, empty_ends)     rows and pairs on proximity_ref.corpus(N, empty_ends), for its VARIANTS
    expected(corpus) -> [5-tuple]   the oracle's answer to every pair of a SnipCorpus, computed once
    random_draws(n, seed)           (stream, terms, weights, span) draws for the CPU comparison of the three formulations

The reference project has no such search: best_window is the oracle, and test_snippet_cases.py holds it against the two
independent formulations on every case and on random draws.  All arithmetic is integer; there is no tolerance anywhere."""
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

from msretr._abi import MSR_PHRASE_MAX_TERMS as LMAX
from msretr._abi import MSR_PROX_MAX_SPAN as SPAN_MAX
from msretr._abi import MSR_SNIPPET_MAX_WEIGHT as WMAX
from phrase_ref import A, B, C_, D, E, F, G, H, L16, L17, N_TERMS, P, Q, UNUSED, X, Y, _index_of
from proximity_ref import VARIANTS  # noqa: F401
from proximity_ref import corpus as near_corpus

NONE = (-1, 0, 0, 0, 0)


def valid(terms, weights, span, n_terms=N_TERMS):
    return (1 <= len(terms) <= LMAX and len(weights) == len(terms) and all(0 <= int(t) < n_terms for t in terms)
            and all(0 <= int(w) <= WMAX for w in weights) and 1 <= span <= SPAN_MAX)


# ------------------------------------------------------------------------------------------ the definition, as plain loops
def best_window(stream, terms, weights, span, n_terms=N_TERMS):
    """(start, cover, hits, mask, term bits) of the best window of `stream`, or NONE.  For every start a the window is
    stream[a : a + span] (cut at the end); hits = its positions that hold a term of the row, cover = the summed weights of
    the distinct ids present (a repeated id: the weight and the bit of its first occurrence); the largest (cover, hits)
    wins, the smallest start among equal ones."""
    if not valid(terms, weights, span, n_terms):
        return NONE
    first = {}
    for j, t in enumerate(terms):
        if int(t) not in first:
            first[int(t)] = j
    best = None
    for a in range(len(stream)):
        hits, seen, mask = 0, [], 0
        for k in range(span):
            if a + k >= len(stream):
                break
            t = stream[a + k]
            if t in first:
                hits += 1
                mask |= 1 << k
                if t not in seen:
                    seen.append(t)
        if hits == 0:
            continue
        cover = sum(int(weights[first[t]]) for t in seen)
        bits = sum(1 << first[t] for t in seen)
        if best is None or (cover, hits) > (best[1], best[2]):               # strictly: the earliest of equal ones stays
            best = (a, cover, hits, mask, bits)
    return NONE if best is None else best


# ------------------------------------------------------------------------------------------ the same by other means
def best_window_2(stream, terms, weights, span, n_terms=N_TERMS):
    """One window that slides: a count per distinct id, cover and hits updated by the token that leaves and the one that
    enters; the winner's mask and bits are read off the stream afterwards."""
    if not valid(terms, weights, span, n_terms):
        return NONE
    weight, bit = {}, {}
    for j in range(len(terms) - 1, -1, -1):                  # downwards: the first occurrence is written last
        weight[int(terms[j])], bit[int(terms[j])] = int(weights[j]), j
    n = len(stream)
    count = dict.fromkeys(weight, 0)
    cover = hits = 0

    def enter(t):
        nonlocal cover, hits
        if t in count:
            hits += 1
            count[t] += 1
            if count[t] == 1:
                cover += weight[t]

    def leave(t):
        nonlocal cover, hits
        if t in count:
            hits -= 1
            count[t] -= 1
            if count[t] == 0:
                cover -= weight[t]

    for i in range(min(span, n)):
        enter(stream[i])
    top, at = None, -1
    for a in range(n):
        if hits > 0 and (top is None or (cover, hits) > top):
            top, at = (cover, hits), a
        leave(stream[a])
        if a + span < n:
            enter(stream[a + span])
    if top is None:
        return NONE
    win = stream[at:at + span]
    return (at, top[0], top[1], sum(1 << k for k, t in enumerate(win) if t in weight), sum({1 << bit[t] for t in win if t in bit}))


def best_windows_fast(tok_off, tok_ids, pair_doc, pair_row, rows, weights, spans, n_terms=N_TERMS):
    """-> (start int32, cover int32, hits int32, mask uint64, terms uint32) arrays, one entry per pair.  Per distinct row the
    pairs' documents are laid end to end; with c_t the prefix count of token t, the window that starts at i and ends before
    hi = min(i + span, the document's end) holds t iff c_t[hi] - c_t[i] > 0, and hits = c_any[hi] - c_any[i]; a segmented
    maximum of cover * 128 + hits and the first position that reaches it give the answer.  (Checked against best_window on
    every case by test_snippet_cases.py.)"""
    off, tok = np.asarray(tok_off, np.int64), np.asarray(tok_ids, np.int64)
    N, n = len(off) - 1, len(pair_doc)
    pd, pr = np.asarray(pair_doc, np.int64).reshape(-1), np.asarray(pair_row, np.int64).reshape(-1)
    o_start, o_cover, o_hits = np.full(n, -1, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    o_mask, o_terms = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
    ok = (pd >= 0) & (pd < N) & (pr >= 0) & (pr < len(rows))
    for r in np.unique(pr[ok]).tolist():
        p, w, span = [int(t) for t in rows[r]], [int(v) for v in weights[r]], int(spans[r])
        if not valid(p, w, span, n_terms):
            continue
        sel = np.nonzero(ok & (pr == r))[0]
        docs = pd[sel]
        lens = off[docs + 1] - off[docs]
        total = int(lens.sum())
        if total == 0:
            continue
        seg = np.repeat(np.arange(len(docs)), lens)
        seg_at = np.cumsum(lens) - lens
        i = np.arange(total)
        local = i - seg_at[seg]
        t = tok[off[docs][seg] + local]
        hi = np.minimum(i + span, (seg_at + lens)[seg])
        count = lambda is_t: np.concatenate([[0], np.cumsum(is_t)])
        cover, any_t, present = np.zeros(total, np.int64), np.zeros(total, bool), {}
        for j, tid in enumerate(p):
            if tid in p[:j]:
                continue
            is_t = t == tid
            c = count(is_t)
            present[j] = c[hi] - c[i] > 0
            cover += w[j] * present[j]
            any_t |= is_t
        c = count(any_t)
        hits = c[hi] - c[i]
        key = np.where(hits > 0, cover * 128 + hits, -1)
        top = np.full(len(docs), -1, np.int64)
        full = lens > 0
        top[full] = np.maximum.reduceat(key, seg_at[full])
        at = np.nonzero((key == top[seg]) & (key >= 0))[0]
        first = np.full(len(docs), total, np.int64)
        np.minimum.at(first, seg[at], at)
        for k in np.nonzero(first < total)[0].tolist():
            a, dst = int(first[k]), sel[k]
            o_start[dst], o_cover[dst], o_hits[dst] = local[a], cover[a], hits[a]
            o_mask[dst] = np.uint64(sum(1 << m for m in np.nonzero(any_t[a:hi[a]])[0].tolist()))
            o_terms[dst] = np.uint32(sum(1 << j for j, pres in present.items() if pres[a]))
    return o_start, o_cover, o_hits, o_mask, o_terms


# ------------------------------------------------------------------------------------------ corpora and cases
@dataclass
class SnipCorpus:
    streams: list                                            # the documents as lists
    ix: object                                               # a postings-only CorpusIndex with the forward index
    tok_off: np.ndarray
    tok_ids: np.ndarray
    rows: list = field(default_factory=list)                 # term ids per row
    weights: list = field(default_factory=list)
    spans: list = field(default_factory=list)
    pairs: list = field(default_factory=list)                # (document, row, the edge the pair claims)

    @property
    def n_docs(self):
        return len(self.streams)

    def row(self, terms, weights, span):
        self.rows.append(list(terms)); self.weights.append(list(weights)); self.spans.append(int(span))
        return len(self.rows) - 1

    def pair(self, doc, row, claim):
        self.pairs.append((int(doc), int(row), claim))


DOC_LENS = (0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193)
ROW_LENS = (1, 4, 5, 8, 9, 16)


def _fill(n):
    return [F] * n


def _doc(n, at):
    s = _fill(n)
    for pos, t in at.items():
        s[pos] = t
    return s


@lru_cache(maxsize=None)
def hand():
    """The hand-made corpus: every document and pair names the edge it is there for.  The LAST document ends the token buffer
    with a term of its row (tok_ids is sized exactly: a read past the document's end would be a read past the buffer)."""
    docs, name = [], {}

    def add(key, s):
        name[key] = len(docs)
        docs.append(list(s))

    for n in DOC_LENS:                                       # A on the first token, B on the last
        add(f"len{n}", _doc(n, {0: A, n - 1: B} if n >= 2 else ({0: A} if n else {})))
    add("at_63_64", _doc(193, {63: A, 64: B}))
    add("at_127_128", _doc(193, {127: A, 128: B}))
    add("third_chunk", _doc(300, {150: A}))                  # the only occurrence in chunk 2 ...
    add("last_chunk", _doc(300, {299: A}))                   # ... and on the last token of the last chunk
    add("tie_0_2", _doc(200, {5: A, 6: B, 140: A, 141: B}))  # equal windows in chunk 0 and chunk 2: the earliest wins
    add("best_2", _doc(200, {5: A, 6: B, 140: A, 141: B, 142: C_}))      # chunk 2 holds one term more
    add("hits_2", _doc(200, {5: A, 6: B, 140: A, 141: B, 142: A}))       # the same cover, one hit more in chunk 2
    add("tie_end", _doc(70, {10: A, 69: A}))                 # a full window and the shorter one at the end: equal
    add("short_best", [F, F, A, F, B])                       # shorter than the span: every window is a shortened one
    add("end_better", _doc(70, {10: A, 68: A, 69: B}))       # the best window ends on the document's last token
    add("before_terms", [F, F, A])                           # its successor begins with the row's other terms
    add("starts_terms", [B, C_, A, F, F, F])
    add("empty_between", [])
    add("l16", _fill(3) + L16 + _fill(2))
    wide = _fill(64)
    for j, t in enumerate(L16):
        wide[63 if j == 15 else 4 * j] = t
    add("l16_wide", _fill(40) + wide + _fill(30))            # 16 distinct ids over exactly 64 tokens, from position 40 to 103
    add("l17", L17)
    add("repeat", [F, A, F, B, A, F, F, F, F, B])
    add("pq", [P, Q, F, P, Q, P, F, F, Q])
    add("zero", [F, A, F, F, A, B, F])
    add("long", _doc(1000, {70: G, 500: G, 505: H, 506: E, 990: G, 995: H}))
    add("last", [Y, F, A, B, F, X])                          # the stream's last token is X
    N = len(docs)
    ix, off, tok = _index_of(docs, N)
    c = SnipCorpus(docs, ix, off, tok)
    c.name = name
    d = name.__getitem__
    ab64, ab17, ab2, ab1 = c.row([A, B], [3, 5], 64), c.row([A, B], [3, 5], 17), c.row([A, B], [3, 5], 2), c.row([A, B], [3, 5], 1)
    ba63 = c.row([B, A], [7, 7], 63)
    for n in DOC_LENS:
        for r in (ab64, ab17, ab2, ab1, ba63):
            c.pair(d(f"len{n}"), r, f"a document of {n} tokens, A first and B last, span {c.spans[r]}")
    for key in ("at_63_64", "at_127_128"):
        for r in (ab64, ab2, ab1, ba63):
            c.pair(d(key), r, f"two terms at positions {key[3:]}, span {c.spans[r]}")
    a5, a64 = c.row([A], [9], 5), c.row([A], [9], 64)
    for key in ("third_chunk", "last_chunk"):
        for r in (a5, a64, ab64):
            c.pair(d(key), r, f"the only occurrence in the {key.replace('_', ' ')}, span {c.spans[r]}")
    ab4, abc4, abc64 = c.row([A, B], [3, 5], 4), c.row([A, B, C_], [3, 5, 2], 4), c.row([A, B, C_], [3, 5, 2], 64)
    for key in ("tie_0_2", "best_2", "hits_2"):
        for r in (ab4, abc4, abc64, ab64, ab2):
            c.pair(d(key), r, f"{key}: equal or better windows in chunk 0 and chunk 2, span {c.spans[r]}")
    for r in (a5, a64, c.row([A], [9], 1)):
        c.pair(d("tie_end"), r, "a tie between a full window and the shorter window at the document's end")
    for r in (ab64, ab4, ab2):
        c.pair(d("short_best"), r, "the best window is a shortened one (the document is shorter than the span, or it is not)")
        c.pair(d("end_better"), r, "the best window ends on the document's last token")
    for r in (abc64, abc4, ab64):
        c.pair(d("before_terms"), r, "the successor begins with the row's terms: cover and mask must not see them")
        c.pair(d("starts_terms"), r, "the document that begins with them")
        c.pair(d("empty_between"), r, "a document of length 0")
    xy = c.row([X, Y], [4, 4], 64)
    c.pair(d("last"), xy, "the last document of the buffer: X on the stream's last token")
    c.pair(d("last"), c.row([X], [1], 64), "the last document, a window that starts on the last token at most")
    c.pair(d("last"), c.row([X, A], [4, 4], 3), "the last document, span 3")
    for L in ROW_LENS + (17,):                               # every scan width; 17 terms: no window
        p = L17[:L]
        for span in (1, L, 63, 64, 0, 65):
            r = c.row(p, [1 + 3 * j for j in range(L)], span)
            for key in ("l16", "l16_wide", "l17"):
                c.pair(d(key), r, f"L = {L}, span {span}")
    r = c.row(L16[::-1], [WMAX] * 16, 16)
    c.pair(d("l16"), r, "sixteen terms of weight 1 << 20, all present: cover = 2^24 exactly")
    c.pair(d("l16_wide"), r, "the same row, span 16: not all present")
    r = c.row(L16, [WMAX] * 16, 64)
    c.pair(d("l16_wide"), r, "sixteen terms of weight 1 << 20 over exactly 64 tokens: cover = 2^24")
    c.pair(d("l16"), r, "the same row on the narrow document")
    empty = c.row([], [], 5)
    c.pair(d("zero"), empty, "an empty row: no window")
    for p, w in (([A, B, A], [3, 5, 1000]), ([A, A, B], [3, 1000, 5]), ([B, A, B, A], [5, 3, 0, WMAX + 1]), ([A, A], [0, 7])):
        for span in (2, 5, 64):
            r = c.row(p, w, span)
            c.pair(d("repeat"), r, f"a repeated id {p} {w}: the weight and the bit of its first occurrence, span {span}")
            c.pair(d("zero"), r, f"a repeated id {p} {w}, span {span}")
    for p in ([A, -1], [N_TERMS, A], [-1], [A, B, -7]):
        c.pair(d("zero"), c.row(p, [1] * len(p), 5), f"an id outside [0, n_terms) {p}: no window")
    for w in ([0, 5], [WMAX, 5], [WMAX + 1, 5], [-1, 5], [5, WMAX + 1], [0, 0], [WMAX, WMAX]):
        for span in (3, 64):
            c.pair(d("zero"), c.row([A, B], w, span), f"weights {w}, span {span} (all 0: hits decide, the start is >= 0)")
    for p, w in (([P, Q], [0, 0]), ([P, Q], [2, 1]), ([Q, P], [2, 1]), ([P, Q, P], [1, 1, 50])):
        for span in (1, 2, 3, 4, 64):
            c.pair(d("pq"), c.row(p, w, span), f"P Q F P Q P F F Q with {p} {w}, span {span}")
    for p, w, span in (([G, H], [5, 6], 6), ([G, H, E], [5, 6, 7], 64), ([H, E, G], [1, 1, 1], 7), ([E], [0], 1), ([G], [1], 64),
                       ([UNUSED], [9], 64), ([UNUSED, G], [9, 1], 10)):
        c.pair(d("long"), c.row(p, w, span), f"1000 tokens (16 chunks, every one is read): {p} {w}, span {span}")
    return c


@lru_cache(maxsize=None)
def corpus_cases(N, empty_ends=False):
    """proximity_ref.corpus(N, empty_ends) with rows of its named terms and pairs on its planted and its random documents."""
    nc = near_corpus(N, empty_ends)
    c = SnipCorpus(nc.streams, nc.ix, nc.tok_off, nc.tok_ids)
    c.name = nc.doc
    rows = [c.row([A, B], [3, 5], 17), c.row([A, B, C_], [3, 5, 2], 64), c.row([B, A], [1, 1], 2), c.row([C_, D], [4, 6], 64),
            c.row([C_, D], [4, 6], 16), c.row([X, Y], [2, 2], 64), c.row([P, Q, P], [2, 3, 9], 3), c.row([X], [1], 1),
            c.row([UNUSED], [5], 64), c.row(L16, list(range(1, 17)), 16), c.row(L16[:9], [7] * 9, 64), c.row(L16[:5], [0] * 5, 5),
            c.row([3, 7, 11, 3], [10, 20, 30, 40], 8), c.row(list(range(0, 16)), [1 << j for j in range(16)], 30),
            c.row([A, -1], [1, 1], 5), c.row([A, B], [1, 1], 65), c.row([], [], 5)]
    gh, heg, ghe = c.row([G, H], [5, 6], 64), c.row([H, E, G], [1, 2, 3], 64), c.row([G, H, E], [1, 1, 1], 3)
    lens = np.diff(nc.tok_off)
    short = [int(x) for x in np.nonzero(lens <= 200)[0]]
    some = short if N <= 33 else sorted(set(short[:24] + short[-24:] + [x for x in short if x in nc.doc.values()]))
    for r in rows:
        for doc in some:
            c.pair(doc, r, f"document {doc}, row {c.rows[r]} span {c.spans[r]}")
    for doc in [int(x) for x in np.nonzero(lens > 200)[0]]:  # the long planted documents: a few rows each
        for r in (gh, heg, ghe):
            c.pair(doc, r, f"a document of {int(lens[doc])} tokens, row {c.rows[r]} span {c.spans[r]}")
    return c


@lru_cache(maxsize=None)
def _expected(key):
    c = hand() if key == "hand" else corpus_cases(*key)
    return [best_window(c.streams[d], c.rows[r], c.weights[r], c.spans[r]) for d, r, _ in c.pairs]


def expected(key="hand"):
    """The oracle's answer to every pair of hand() (key "hand") or corpus_cases(N, empty_ends) (key (N, empty_ends)):
    computed once, shared by the tests."""
    return _expected(key)


def random_draws(n, seed=3):
    """n draws of (stream, terms, weights, span): streams of 0 .. 200 tokens over 12 ids (so that rows meet them), rows of
    1 .. 16 terms with repeats, weights with zeros and the maximum, every span; one draw in nine is an invalid row."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        length = int(rng.integers(0, 201)) if i % 4 == 0 else int(rng.integers(0, 70))
        density = (0.05, 0.3, 1.0)[i % 3]
        s = np.where(rng.random(length) < density, rng.integers(0, 12, length), F).tolist()
        L = int(rng.integers(1, 17))
        p = rng.integers(0, 12 if i % 5 else 20, L).tolist()
        w = rng.choice([0, 1, 2, 3, 1000, WMAX], L).tolist() if i % 2 else rng.integers(0, 5, L).tolist()
        span = int(rng.integers(1, 65))
        if i % 9 == 8:
            kind = (i // 9) % 6
            if kind == 0: p = p + list(range(20, 20 + 17 - L))
            elif kind == 1: p[int(rng.integers(0, L))] = -1
            elif kind == 2: p[int(rng.integers(0, L))] = N_TERMS
            elif kind == 3: w[int(rng.integers(0, L))] = WMAX + 1
            elif kind == 4: span = (0, 65, -3)[i % 3]
            else: w[int(rng.integers(0, L))] = -1
            if kind == 0:
                w = w + [1] * (len(p) - len(w))
        out.append((s, p, w, span))
    return out
