"""Shared cases and the plain Python reference of proximity search (msr_proximity_sets, DESIGN K13).

    near_mask(streams, phrase, span, ordered, cand_mask, n_terms) -> bool [N]   the two definitions of msretr.h, loops over documents
    near_mask_2(...)                                                            the same by other means: a sliding window with counts
                                                                                (any order), a DP over positions (ordered)
    near_mask_fast(tok_off, tok_ids, ...)                                       the same over the whole stream at once (numpy)
    corpus(N, empty_ends=False) -> NearCorpus                                   phrase_ref's corpus with further planted documents
    row_cases(c) -> [NearCase]                                                  rows (terms, span, ordered, candidate row) and the
                                                                                edge each one claims
    expected(N, empty_ends) -> (cases, masks)                                   the oracle's answer, computed once per corpus

The reference project has no proximity search: near_mask is the oracle, and test_proximity_cases.py holds it against the two
independent formulations on every case and on random rows.  The corpora are phrase_ref's (the sizes straddle a bitset word, a
skip-table tile and the kernel's span of S documents, and every document it plants is still there, at its index); the
documents planted here stand at indices phrase_ref leaves to random ones (23 .. 30, then 33 ..), so the 33-document corpus
holds the first eight of them and the 1-document corpus none."""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from msretr._abi import MSR_PROX_MAX_SPAN as SPAN_MAX
from phrase_ref import (A, B, BIG, C_, D, E, F, G, H, L16, L17, LMAX, N_RANDOM, N_TERMS, P, Q, S, SIZES, UNUSED, X, Y,  # noqa: F401
                        PhraseCorpus, _index_of, cand_mask, phrase_mask)
from phrase_ref import corpus as phrase_corpus
from phrase_ref import row_cases as phrase_row_cases

VARIANTS = [(1, False), (33, False), (33, True), (1025, False), (1025, True), (S + 1, False), (BIG, False)]
RANDOM_SPANS = ("L", "L+1", "L+3", 20, 64)


def _valid(p, span, n_terms):
    return 1 <= len(p) <= LMAX and all(0 <= t < n_terms for t in p) and 1 <= span <= SPAN_MAX


# ------------------------------------------------------------------------------------------ the definitions, as plain loops
def _follow(s, p, j, prev, stop):
    """Is there a position for p[j], p[j + 1], ... after `prev` and below `stop`, in this order?  (Every choice is tried.)"""
    if j == len(p):
        return True
    for i in range(prev + 1, min(stop, len(s))):
        if s[i] == p[j] and _follow(s, p, j + 1, i, stop):
            return True
    return False


def ordered_match(s, p, span):
    """positions i_0 < i_1 < ... < i_{L-1} inside s with s[i_j] == p[j] and i_{L-1} - i_0 + 1 <= span"""
    i0 = -1
    while True:
        try:
            i0 = s.index(p[0], i0 + 1)                       # every start
        except ValueError:
            return False
        if _follow(s, p, 1, i0, i0 + span):
            return True


def any_order_match(s, p, span):
    """one position per distinct id of p, all inside s, with max - min + 1 <= span: some window of `span` tokens holds them all"""
    T = set(p)
    if not all(t in s for t in T):
        return False
    return any(all(t in s[i:i + span] for t in T) for i in range(len(s)))


def near_mask(streams, phrase, span, ordered, cand_mask=None, n_terms=N_TERMS):
    """bool [N]: the candidate documents whose OWN stream matches the row.  A row whose phrase is empty, longer than
    MSR_PHRASE_MAX_TERMS or holds an id outside [0, n_terms), or whose span is outside 1 .. MSR_PROX_MAX_SPAN, matches nothing;
    cand_mask None = every document."""
    N, p = len(streams), [int(t) for t in phrase]
    out = np.zeros(N, bool)
    if not _valid(p, span, n_terms):
        return out
    match = ordered_match if ordered else any_order_match
    for d in (range(N) if cand_mask is None else np.nonzero(cand_mask)[0].tolist()):
        out[d] = match(streams[d], p, span)
    return out


# ------------------------------------------------------------------------------------------ the same by other means
def ordered_match_2(s, p, span):
    """DP over positions: start[j] = the LATEST start of a match of p[0 .. j] that ends before the current position (a later
    start never makes a longer span, whatever follows); j runs downwards so that one position serves one term."""
    L = len(p)
    start = [-1] * L
    for i, t in enumerate(s):
        for j in range(L - 1, -1, -1):
            if t == p[j]:
                if j == 0:
                    start[0] = i
                elif start[j - 1] >= 0:
                    start[j] = max(start[j], start[j - 1])
                if j == L - 1 and start[j] >= 0 and i - start[j] + 1 <= span:
                    return True
    return False


def any_order_match_2(s, p, span):
    """The shortest window that holds every distinct id: two pointers with a count per id."""
    need = set(p)
    have, missing, left = dict.fromkeys(need, 0), len(need), 0
    for right, t in enumerate(s):
        if t in have:
            have[t] += 1
            missing -= have[t] == 1
        while missing == 0:
            if right - left + 1 <= span:
                return True
            u = s[left]
            if u in have:
                have[u] -= 1
                missing += have[u] == 0
            left += 1
    return False


def near_mask_2(streams, phrase, span, ordered, cand_mask=None, n_terms=N_TERMS):
    N, p = len(streams), [int(t) for t in phrase]
    out = np.zeros(N, bool)
    if not _valid(p, span, n_terms):
        return out
    match = ordered_match_2 if ordered else any_order_match_2
    for d in (range(N) if cand_mask is None else np.nonzero(cand_mask)[0].tolist()):
        s = streams[d]
        out[d] = all(t in s for t in p) and match(s, p, span)
    return out


_FAR = 1 << 60


def near_mask_fast(tok_off, tok_ids, phrase, span, ordered, cand_mask=None, n_terms=N_TERMS):
    """Over the whole stream at once: nxt_t[i] = the first position >= i that holds t.  Any order: the window that starts at i
    ends at max over t of nxt_t[i]; ordered: from every start, term after term to the next occurrence.  The end must lie in
    i's document and at most span - 1 behind i.  (Checked against near_mask on every case by test_proximity_cases.py.)"""
    off, tok = np.asarray(tok_off, np.int64), np.asarray(tok_ids, np.int64)
    N, T, p = len(off) - 1, len(tok), [int(t) for t in phrase]
    out = np.zeros(N, bool)
    if not _valid(p, span, n_terms) or T == 0:
        return out
    i = np.arange(T)
    doc = np.repeat(np.arange(N), np.diff(off))

    def nxt(t):
        at = np.where(tok == t, i, _FAR)
        return np.append(np.minimum.accumulate(at[::-1])[::-1], _FAR)

    if ordered:
        end = np.where(tok == p[0], i, _FAR)
        for t in p[1:]:
            end = np.where(end < _FAR, nxt(t)[np.minimum(end + 1, T)], _FAR)
    else:
        end = np.max([nxt(t)[:T] for t in set(p)], axis=0)
    ok = (end < off[doc + 1]) & (end - i + 1 <= span)
    out[doc[ok]] = True
    return out if cand_mask is None else out & np.asarray(cand_mask, bool)


# ------------------------------------------------------------------------------------------ corpus and cases
@dataclass
class NearCorpus(PhraseCorpus):
    streams: list = None                                     # the documents as lists (what near_mask walks)


@dataclass
class NearCase:
    phrase: list
    span: int
    ordered: bool
    cand: int                                                # row_cand value (-1, a row, or n_cand)
    claim: str


GAP_SPANS = (2, 3, 17, 64)
GEO_AT = (0, 1, 62, 63, 64, 65, 127)
GEO_SPANS = (2, 17, 64)
END_LENS = ((63, 17), (64, 64), (65, 64), (128, 17), (129, 64), (4097, 64), (10000, 17))      # (document length, span)


def _gap3(extent):
    """A .. B .. C over exactly `extent` tokens (B about half way)."""
    k = extent - 3
    return [A] + [F] * (k // 2) + [B] + [F] * (k - k // 2) + [C_]


def _planted():
    """(name, stream) in planting order: the first eight are what the 33-document corpus holds."""
    fill = lambda n: [F] * n
    docs = [("g2_fit_3", [F, F, A, F, B, F]), ("g2_long_3", [F, F, A, F, F, B, F]),
            ("geo_63_17", fill(63) + [C_] + fill(15) + [D] + fill(3)),
            ("trap_abc", [A, B] + fill(70) + [A, F, B, C_]), ("trap_aab", [A, F, F, F, A, A, B]),
            ("pfp", [P, F, P]), ("pqfp", [P, Q, F, P]), ("affb", [A, F, F, B])]
    for sp in GAP_SPANS:                                     # two terms whose extent is exactly sp / sp + 1
        if sp != 3:
            docs.append((f"g2_fit_{sp}", [F, F, A] + fill(sp - 2) + [B, F]))
            docs.append((f"g2_long_{sp}", [F, F, A] + fill(sp - 1) + [B, F]))
        if sp >= 3:                                          # three terms
            docs.append((f"g3_fit_{sp}", [F] + _gap3(sp) + [F]))
            docs.append((f"g3_long_{sp}", [F] + _gap3(sp + 1) + [F]))
    for at in GEO_AT:                                        # first term at stream position `at`, last term sp - 1 further on
        for sp in GEO_SPANS:
            if (at, sp) != (63, 17):
                docs.append((f"geo_{at}_{sp}", fill(at) + [C_] + fill(sp - 2) + [D] + fill(3)))
    for n, sp in END_LENS:                                   # the match ends on the last token of a document of n tokens
        docs.append((f"end_{n}", fill(n - sp) + [G] + fill(sp - 2) + [H]))
    # the first term in chunk c, the next term first seen in chunk c + 2: too far apart for any span
    docs.append(("skip_129", fill(60) + [G] + fill(67) + [H]))
    docs.append(("skip_4097", fill(4000) + [G] + fill(95) + [H]))
    docs.append(("skip_10000", fill(100) + [G] + fill(9898) + [H]))       # no match in 10 000 tokens: every chunk is read
    docs.append(("one_p", [F, P, F]))
    docs.append(("bafa", [B, A, F, A]))
    wide = fill(64)
    for j, t in enumerate(L16):
        wide[63 if j == 15 else 4 * j] = t
    docs.append(("l16_wide", wide))                          # 16 distinct ids over exactly 64 tokens, in order
    return docs


@lru_cache(maxsize=None)
def corpus(N, empty_ends=False):
    base = phrase_corpus(N, empty_ends)
    tok = base.tok_ids.tolist()
    streams = [tok[int(base.tok_off[d]):int(base.tok_off[d + 1])] for d in range(N)]
    taken, doc = set(base.doc.values()), dict(base.doc)
    free = (d for d in range(23, N) if d not in taken)
    for name, s in _planted():
        d = next(free, None)
        if d is None:
            break
        assert name not in doc
        doc[name] = d
        streams[d] = list(s)
    ix, off, tok_ids = _index_of(streams, N)
    cands = list(base.cands)
    for name, d in doc.items():
        if name not in base.doc:
            m = np.zeros(N, bool)
            m[d] = True
            cands.append(("only_" + name, m))
    return NearCorpus(N, ix, off, tok_ids, doc, cands, streams)


def row_cases(c):
    """The rows every corpus is asked for; a case whose planted document the corpus lacks (it is too small) is left out."""
    R, nc = [], len(c.cands)
    names = [n for n, _ in c.cands]

    def add(phrase, span, ordered, cand, claim):
        if isinstance(cand, str):
            if cand not in names:
                return
            cand = names.index(cand)
        R.append(NearCase(list(phrase), int(span), bool(ordered), cand, claim))

    def both(phrase, span, cand, claim):
        add(phrase, span, True, cand, "ordered: " + claim)
        add(phrase, span, False, cand, "any order: " + claim)

    # ordered, span == L: the exact phrase (every row of phrase_ref, the invalid ones too)
    for r in phrase_row_cases(c):
        add(r.phrase, len(r.phrase), True, r.cand, "ordered, span == L: " + r.claim)
    # the gap exactly fits / is one too long
    for sp in GAP_SPANS:
        both([A, B], sp, f"only_g2_fit_{sp}", f"two terms over exactly span = {sp} tokens")
        both([A, B], sp, f"only_g2_long_{sp}", f"two terms over span + 1 = {sp + 1} tokens: no match")
        add([B, A], sp, False, f"only_g2_fit_{sp}", f"any order: the terms in reverse order, span {sp}")
        add([B, A], sp, True, f"only_g2_fit_{sp}", f"ordered: the terms in reverse order, span {sp}: no match")
        add([A, B, A], sp, False, f"only_g2_fit_{sp}", f"any order: A B A equals A B (a repeated id counts once), span {sp}")
        add([A, B, A], sp, False, f"only_g2_long_{sp}", f"any order: A B A equals A B, one too long at span {sp}")
        both([A, B, C_], sp, f"only_g3_fit_{sp}", f"three terms over exactly span = {sp} tokens")
        both([A, B, C_], sp, f"only_g3_long_{sp}", f"three terms over span + 1 = {sp + 1} tokens: no match")
        add([C_, A, B], sp, False, f"only_g3_fit_{sp}", f"any order: three terms rotated, span {sp}")
    both([A, B], 17, -1, "A .. B within 17 tokens over the corpus")
    both([A, B, C_], 64, "rnd", "A .. B .. C within 64 tokens inside a candidate row")
    # chunk geometry
    for at in GEO_AT:
        for sp in GEO_SPANS:
            both([C_, D], sp, f"only_geo_{at}_{sp}", f"first term at stream position {at}, last term {sp - 1} further on")
            both([C_, D], sp - 1, f"only_geo_{at}_{sp}", f"first term at {at}, span {sp - 1} is one too short: no match")
            add([D, C_], sp, False, f"only_geo_{at}_{sp}", f"any order, reversed: first term at {at}, span {sp}")
    both([C_, D], 64, "only_geo_0_64", "span 64 starting at lane 0: all inside one chunk")
    both([C_, D], 64, "only_geo_1_64", "span 64 starting at lane 1: the last term is bit 0 of the next chunk's mask")
    both([C_, D], 64, "only_geo_63_64", "span 64 starting at lane 63: the last term is bit 62 of the next chunk's mask")
    both([C_, D], 64, -1, "C .. D within 64 tokens over the corpus")
    for n, sp in END_LENS:
        both([G, H], sp, f"only_end_{n}", f"a document of {n} tokens: the match ends on its last token")
        both([G, H], sp - 1, f"only_end_{n}", f"a document of {n} tokens: one too short, no match")
        both([H, G], sp, f"only_end_{n}", f"a document of {n} tokens, the terms reversed (H stands on the last token)")
    for n in (129, 4097, 10000):
        both([G, H], 64, f"only_skip_{n}", f"first term in chunk c, the next term first seen in chunk c + 2 ({n} tokens): no match")
    both([G, H], 64, -1, "G .. H within 64 tokens over the corpus")
    both([H, E, G], 64, "only_len10000", "phrase_ref's 10 000-token document: H E G never within 64 tokens (every chunk is read)")
    both([G, H, E], 3, "only_len10000", "10 000 tokens: G H E at positions 4095 - 4097")
    # greedy traps, ordered
    add([A, B, C_], 4, True, "only_trap_abc", "A B F x 70 A F B C: the first start fails, a later one matches")
    add([A, B, C_], 3, True, "only_trap_abc", "the same, span 3: no match")
    add([A, B, C_], 64, True, "only_trap_abc", "the same, span 64: the later start")
    add([A, A, B], 3, True, "only_trap_aab", "A F F F A A B: A A B from the second A")
    add([A, A, B], 7, True, "only_trap_aab", "A F F F A A B, span 7: also from the first")
    add([A, A, B], 2, True, "only_trap_aab", "span < L: nothing")
    for sp in (2, 64):
        add([P, P], sp, True, "only_one_p", f"P P on a document with one P, span {sp}: a repeated id needs two positions")
    add([P, P], 64, False, "only_one_p", "any order: P P is P, one P is enough")
    add([P, P], 2, True, "only_pfp", "P P on P F P, span 2: no match")
    add([P, P], 3, True, "only_pfp", "P P on P F P, span 3")
    add([P, Q, P], 3, True, "only_pqfp", "P Q P on P Q F P, span 3: no match")
    add([P, Q, P], 4, True, "only_pqfp", "P Q P on P Q F P, span 4")
    add([P, Q, P], 2, False, "only_pqfp", "any order: P Q P is {P, Q}, span 2")
    add([P, Q, P, Q, P], 5, True, "only_overlap", "the whole document P Q P Q P")
    add([P, P, P], 5, True, "only_overlap", "P P P at positions 0, 2, 4")
    add([P, P, P], 4, True, "only_overlap", "P P P needs five tokens: no match")
    add([Q, Q, Q], 64, True, "only_overlap", "three Q in a document with two")
    # any order
    add([X], 1, False, -1, "|T| = 1: term containment")
    add([X, X], 1, False, -1, "|T| = 1 from a repeated id")
    add([X], 64, False, "odd", "|T| = 1, span 64")
    add([X], 1, True, -1, "ordered L = 1: term containment")
    add([UNUSED], 64, False, -1, "a term without an occurrence")
    both([A, UNUSED], 64, -1, "one of two terms without an occurrence")
    add([A, B], 3, False, "only_affb", "A F F B, span 3: no match")
    add([A, B], 4, False, "only_affb", "A F F B, span 4")
    add([B, A], 4, False, "only_affb", "A F F B, reversed terms, span 4")
    add([A, B], 2, False, "only_bafa", "B A F A: the window B A")
    add([A, B], 1, False, "only_bafa", "span < |T|: nothing")
    add([A, B], 2, True, "only_bafa", "ordered A B on B A F A: no match")
    add(L16[::-1], 16, False, "only_l16", "L = 16 distinct ids inside span 16, reversed")
    add(L16[::-1], 15, False, "only_l16", "L = 16 distinct ids, span 15: nothing")
    add(L16[5:] + L16[:5], 64, False, "only_l16_wide", "L = 16 distinct ids over exactly 64 tokens")
    add(L16[5:] + L16[:5], 63, False, "only_l16_wide", "L = 16 over 64 tokens, span 63: no match")
    add(L16, 64, True, "only_l16_wide", "ordered L = 16 over exactly 64 tokens")
    add(L16, 63, True, "only_l16_wide", "ordered L = 16, span 63: no match")
    add(L16[::-1], 64, True, "only_l16_wide", "ordered L = 16 reversed: no match")
    add(L16, 20, True, -1, "ordered L = 16, span 20, over the corpus")
    add(L16[:9], 64, False, -1, "nine terms (the widest scan) over the corpus")
    add(L16[:5], 5, True, -1, "five terms (the middle scan), the exact phrase")
    add(L16[:8], 9, True, "only_l16", "eight terms with one token of slack")
    # boundaries
    for cand in ("only_bound_a", "only_bound_b"):
        both([X, Y], 64, cand, "X | Y across the boundary of documents d and d + 1, one of them the only candidate: no match")
        both([Y, X], 5, cand, "the same, reversed")
    both([G, H], 64, "only_short", "a document shorter than L (the next document starts with the second term)")
    both([G, H], 64, "only_after_short", "the next document alone")
    both([G, G], 64, "only_short", "G G on the one-token document G")
    add([X, Y], 5, True, "only_last", "X is the stream's last token and the row's first term: a read past the buffer would be the bug")
    add([X, Y], 64, True, "only_last", "the same at span 64")
    add([X, Y], 6, False, "only_last", "any order: Y .. X over the whole last document")
    add([X, Y], 5, False, "only_last", "any order: one too short")
    add([X, A], 4, False, "only_last", "any order: A .. X ending on the stream's last token")
    for name in ("only_empty_first", "only_empty_5", "only_empty_22", "only_empty_last"):
        both([A], 64, name, "a document of length 0")
        both([A, B], 64, name, "a document of length 0, two terms")
    # invalid rows: EMPTY, with and without a candidate row
    for cand in (-1, "odd"):
        for sp in (0, -1, 65):
            both([A, B], sp, cand, f"span {sp}: empty row")
        both([], 1, cand, "L = 0: empty row")
        both(L17, 64, cand, "L = 17: empty row")
        both([A, -1], 5, cand, "an id of -1: empty row")
        both([N_TERMS, A], 5, cand, "an id of n_terms: empty row")
    # candidate rules
    both([A, B], 5, -1, "row_cand -1: every document")
    both([A, B], 5, "odd", "a candidate row (its bits at or above N are set on the device)")
    both([A, B], 5, nc, "row_cand == n_cand: empty row")
    both([A, B], 5, -2, "row_cand below -1: empty row")
    both([A, B], 5, "none", "an empty candidate row")
    both([A, B], 5, "edges", "candidate documents at bits 0, 31, 32, 1023, 1024, S - 1, S, N - 1")
    both([B, A], 20, "edges", "the same, reversed and wider")
    # rows of the random documents
    rng = np.random.default_rng(11)
    lens = np.diff(c.tok_off)
    for d in np.nonzero((lens >= 8) & (lens <= 40))[0][:40:8]:
        s = c.streams[d]
        both([s[1], s[4]], 4, -1, f"two terms of document {d}, two tokens between them")
        both([s[5], s[2], s[0]], 6, "rnd", f"three terms of document {d}, out of order")
        both([s[0], s[-1]], len(s), "odd", f"the first and the last term of document {d}")
    for i in range(6):
        both(rng.integers(0, N_RANDOM, 2).tolist(), (3, 20, 64)[i % 3], ("rnd", -1, "odd")[i % 3], f"random pair {i}")
    return R


def random_rows(c, n, seed=5):
    """n rows of 1 .. 4 terms: drawn, taken from a document (in order or not), planted or invalid ones; spans from L, L + 1,
    L + 3, 20 and 64 (L = the number of terms); both modes; any row_cand."""
    rng = np.random.default_rng(seed)
    fixed = [[A, B], [C_, D], [X, Y], [P, Q, P], [G, H], [], [A, -1], L17, [X], [A, B, C_], [B, A], [P, P]]
    lens = np.diff(c.tok_off)
    long = np.nonzero((lens >= 6) & (lens <= 64))[0]
    rows = []
    for i in range(n):
        kind = i % 4
        if kind == 0:
            p = fixed[(i // 4) % len(fixed)]
        elif kind == 1 and len(long):
            s = c.streams[int(long[rng.integers(0, len(long))])]
            at = np.sort(rng.choice(len(s), int(rng.integers(2, 5)), replace=False))
            p = [s[j] for j in (at if i % 8 == 1 else rng.permutation(at))]
        else:
            p = rng.integers(0, N_RANDOM, int(rng.integers(1, 5))).tolist()
        sp = RANDOM_SPANS[int(rng.integers(0, len(RANDOM_SPANS)))]
        sp = {"L": len(p), "L+1": len(p) + 1, "L+3": len(p) + 3}.get(sp, sp)
        rows.append(NearCase(p, sp, bool(rng.integers(0, 2)), int(rng.integers(-1, 4)) if i % 5 else len(c.cands), f"random row {i}"))
    return rows


def mask_of(c, r, fn=near_mask):
    """The oracle's answer to one case (fn: near_mask, near_mask_2 or near_mask_fast)."""
    if fn is near_mask_fast:
        return fn(c.tok_off, c.tok_ids, r.phrase, r.span, r.ordered, cand_mask(c, r.cand))
    return fn(c.streams, r.phrase, r.span, r.ordered, cand_mask(c, r.cand))


@lru_cache(maxsize=None)
def expected(N, empty_ends=False):
    """(cases, [bool [N]] the oracle's mask of each) of a corpus: computed once, shared by the tests, never changed."""
    c = corpus(N, empty_ends)
    cases = row_cases(c)
    want = [mask_of(c, r) for r in cases]
    for w in want:
        w.setflags(write=False)
    return cases, want
