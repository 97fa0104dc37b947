"""Shared cases and the plain Python reference of phrase search (msr_phrase_sets / msr_combine_sets, DESIGN K12).

    phrase_mask(tok_off, tok_ids, phrase, cand_mask, n_terms) -> bool [N]   the definition of msretr.h, a loop over documents
    phrase_mask_fast(...)                                                   the same over the whole stream at once (numpy)
    combine_mask(masks, and_rows, not_rows, N) -> bool [N]                  msr_combine_sets' conventions
    corpus(N, empty_ends=False) -> PhraseCorpus                             a hand-made index with a forward index and planted documents
    row_cases(c) -> [RowCase]                                               rows (phrase, candidate row) and the edge each one claims

The reference project has no phrase search: this restatement is the oracle, and test_phrase_cases.py checks it against an
independent formulation (documents rendered as strings).  The corpus sizes straddle a bitset word (32), a skip-table tile
(1024) and the kernel's span (S = MSR_TERMSET_SPAN_DOCS)."""
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

from msretr._abi import MSR_PHRASE_MAX_TERMS as LMAX
from msretr._abi import MSR_TERMSET_SPAN_DOCS as S
from msretr.index import CorpusIndex

SIZES = [1, 33, 1025, S + 1, 2 * S + 37]
BIG = 2 * S + 37
N_RANDOM = 50                                                # random documents draw from term ids [0, N_RANDOM)
A, B, C_, D, E, F, G, H, P, Q, X, Y = range(50, 62)          # named terms of the planted documents (F: filler, in no phrase)
L16 = list(range(62, 78))                                    # 16 distinct ids; L17 = L16 + [78]
L17 = L16 + [78]
UNUSED = 79                                                  # a valid id without an occurrence
N_TERMS = 80


def phrase_mask(tok_off, tok_ids, phrase, cand_mask=None, n_terms=N_TERMS):
    """bool [N]: the candidate documents whose OWN stream holds `phrase` at consecutive positions.  A phrase that is empty,
    longer than MSR_PHRASE_MAX_TERMS or holds an id outside [0, n_terms) matches nothing; cand_mask None = every document."""
    N, p = len(tok_off) - 1, [int(t) for t in phrase]
    out = np.zeros(N, bool)
    if not 1 <= len(p) <= LMAX or any(not 0 <= t < n_terms for t in p):
        return out
    tok = tok_ids.tolist() if hasattr(tok_ids, "tolist") else list(tok_ids)
    for d in (range(N) if cand_mask is None else np.nonzero(cand_mask)[0].tolist()):
        s = tok[int(tok_off[d]):int(tok_off[d + 1])]
        out[d] = any(s[i:i + len(p)] == p for i in range(len(s) - len(p) + 1))
    return out


def phrase_mask_fast(tok_off, tok_ids, phrase, cand_mask=None, n_terms=N_TERMS):
    """phrase_mask over the whole stream at once: position i starts a match iff tok[i + j] == p[j] for every j and i + L does
    not pass the end of i's document (checked against phrase_mask on every case by test_phrase_cases.py)."""
    off, tok = np.asarray(tok_off, np.int64), np.asarray(tok_ids, np.int64)
    N, L = len(off) - 1, len(phrase)
    out = np.zeros(N, bool)
    if not 1 <= L <= LMAX or any(not 0 <= int(t) < n_terms for t in phrase) or len(tok) < L:
        return out
    doc = np.repeat(np.arange(N), np.diff(off))
    i = np.arange(len(tok) - L + 1)
    ok = i + L <= off[doc[i] + 1]
    for j, t in enumerate(phrase):
        ok &= tok[i + j] == int(t)
    out[doc[i[ok]]] = True
    return out if cand_mask is None else out & np.asarray(cand_mask, bool)


def combine_mask(masks, and_rows, not_rows, N):
    """bool [N]: AND of the listed rows AND NOT any listed row.  An empty AND list = every document; a row index outside
    [0, len(masks)) empties the row in the AND list and is ignored in the NOT list."""
    out = np.ones(N, bool)
    for r in and_rows:
        out &= masks[r] if 0 <= r < len(masks) else np.zeros(N, bool)
    for r in not_rows:
        if 0 <= r < len(masks):
            out &= ~masks[r]
    return out


@dataclass
class PhraseCorpus:
    n_docs: int
    ix: CorpusIndex
    tok_off: np.ndarray
    tok_ids: np.ndarray
    doc: dict                                                # name -> document index of a planted document
    cands: list = field(default_factory=list)                # [(name, bool [N])] candidate rows, in row order

    def cand(self, name):
        return [n for n, _ in self.cands].index(name)


@dataclass
class RowCase:
    phrase: list
    cand: int                                                # row_cand value (-1, a row, or n_cand)
    claim: str


def _index_of(streams, N):
    """A postings-only CorpusIndex whose tables agree with the streams (documents without tokens have doc_len 0 and no row)."""
    lens = np.array([len(s) for s in streams], np.int64)
    off = np.zeros(N + 1, np.int64)
    off[1:] = np.cumsum(lens)
    tok = np.fromiter((t for s in streams for t in s), np.int32, count=int(off[-1]))
    key = tok.astype(np.int64) * N + np.repeat(np.arange(N), lens)
    uniq, tf = np.unique(key, return_counts=True)
    term_off = np.zeros(N_TERMS + 1, np.int64)
    term_off[1:] = np.cumsum(np.bincount(uniq // N, minlength=N_TERMS))
    rows = lens[lens > 0]
    ix = CorpusIndex(doc_ids=np.arange(N, dtype=np.int64) * 3 + 7, doc_len=lens.astype(np.int32), term_off=term_off,
                     post_doc=(uniq % N).astype(np.int32), post_tf=tf.astype(np.int32),
                     idf=np.linspace(0.5, 2.0, N_TERMS).astype(np.float32), avgdl=float(np.float32(rows.mean())),
                     total_docs=len(rows), tok_off=off, tok_ids=tok)
    ix.n_docs_global = N
    return ix, off, tok


@lru_cache(maxsize=None)
def corpus(N, empty_ends=False):
    rng = np.random.default_rng(2000 + N + int(empty_ends))
    streams = [rng.integers(0, N_RANDOM, int(rng.integers(0, 41))).tolist() for _ in range(N)]
    doc = {}

    def plant(name, d, s):
        if 0 <= d < N and d not in doc.values():
            doc[name] = d
            streams[d] = list(s)

    first, last = (1, N - 2) if empty_ends else (0, N - 1)
    if N == 1:
        plant("only", 0, [A, B, F, A, B, C_, D, A])          # A B at position 0, D A on the last token, A then nothing
    else:
        if empty_ends:
            plant("empty_first", 0, [])
            plant("empty_last", N - 1, [])
        plant("first", first, [A, B] + rng.integers(0, N_RANDOM, 7).tolist())          # the phrase at position 0
        plant("last", last, [Y, F, A, B, F, X])              # the stream's last token is X: X Y would run past the buffer
        fill = lambda n: [F] * n
        plant("p62_2", 2, fill(62) + [C_, D])                # 64 tokens: ends on the last lane of the first chunk
        plant("p63_2", 3, fill(63) + [C_, D])                # 65 tokens: straddles two chunks
        plant("p64_2", 4, fill(64) + [C_, D] + fill(63))     # 129 tokens: starts the second chunk
        plant("empty_5", 5, [])
        plant("p62_3", 6, fill(62) + [C_, D, E] + fill(63))  # 128 tokens
        plant("p63_3", 7, fill(63) + [C_, D, E])
        plant("p64_3", 8, fill(64) + [C_, D, E])
        plant("len63", 9, fill(61) + [D, E])                 # 63 tokens: ends on the document's last token
        plant("len4097", 10, fill(4095) + [G, H])
        plant("len10000", 11, fill(4095) + [G, H, E] + fill(10000 - 4100) + [H, G])
        plant("overlap", 12, [P, Q, P, Q, P])
        plant("repeat", 13, [Q, P, P])
        plant("late", 14, [A, B, F, A, B, C_])               # A B C: a prefix match at 0, the real one at 3
        plant("prefix_only", 15, [A, B, F, A, B])
        plant("bound_a", 16, [F, F, X])                      # X | Y across the boundary of documents 16 and 17
        plant("bound_b", 17, [Y, F])
        plant("short", 18, [G])                              # G | H: the phrase is longer than the document
        plant("after_short", 19, [H, F, F])
        plant("l16", 20, fill(3) + L16 + fill(2))
        plant("l17", 21, L17)
        plant("empty_22", 22, [])
        for d in (31, 32, 1023, 1024, S - 1, S):
            r = rng.integers(0, N_RANDOM, 9).tolist()
            plant(f"edge_{d}", d, r + [A, B] if d == 31 else r[:4] + [A, B] + r[4:])   # document 31: ends on the last token
    ix, off, tok = _index_of(streams, N)
    edges = np.zeros(N, bool)
    edges[[d for d in (0, 31, 32, 1023, 1024, S - 1, S, N - 1) if d < N]] = True
    cands = [("odd", np.arange(N) % 2 == 1), ("edges", edges), ("rnd", rng.random(N) < 0.5), ("none", np.zeros(N, bool))]
    for name, d in doc.items():
        m = np.zeros(N, bool)
        m[d] = True
        cands.append(("only_" + name, m))
    return PhraseCorpus(N, ix, off, tok, doc, cands)


def row_cases(c):
    """The rows every corpus is asked for; a case whose planted document the corpus lacks (it is too small) is left out."""
    R, nc = [], len(c.cands)
    names = [n for n, _ in c.cands]

    def add(phrase, cand, claim):
        if isinstance(cand, str):
            if cand not in names:
                return
            cand = names.index(cand)
        R.append(RowCase(list(phrase), cand, claim))

    add([A, B], -1, "phrase at position 0 (first document), on the last token (document 31), candidates at bits 0 .. N - 1")
    add([A, B], "edges", "candidate documents at bits 0, 31, 32, 1023, 1024, S - 1, S, N - 1")
    add([A, B], "odd", "a candidate row (its bits at or above N are set on the device)")
    add([A, B], nc, "row_cand == n_cand: empty row")
    add([A, B], -2, "row_cand below -1: empty row")
    add([A, B], "none", "an empty candidate row")
    add([A, B], "only_first", "phrase at position 0")
    add([A, B], "only_edge_31", "phrase ending on the document's last token")
    add([D, A], "only_only", "N == 1: phrase ending on the last token of the stream")
    add([A, B, C_, D, A], -1, "N == 1: a phrase ending on the last token; elsewhere by chance")
    add([X, Y], -1, "present only across document boundaries (bound_a | bound_b, last | nothing): no match")
    add([X, Y], "only_bound_a", "across the boundary, document d is the candidate")
    add([X, Y], "only_bound_b", "across the boundary, document d + 1 is the candidate")
    add([X, Y], "only_last", "X is the stream's last token: the phrase would run past the buffer")
    add([F, X, Y], "only_last", "three terms, two of them on the stream's last tokens")
    add([F, X], "only_last", "phrase ending on the stream's last token")
    add([G, H], "only_short", "phrase longer than the document (the next document starts with its second term)")
    add([G, H], "only_after_short", "the next document alone")
    add([G], "only_short", "L = 1 on a one-token document")
    add([X], -1, "L = 1: term containment")
    add([UNUSED], -1, "L = 1, a term without an occurrence")
    add([A, B], "only_empty_5", "a document of length 0")
    add([A], "only_empty_first", "the first document has length 0")
    add([X], "only_empty_last", "the last document has length 0")
    add(L16, -1, "L = 16")
    add(L16, "only_l17", "L = 16 inside the 17-term document")
    add(L17, -1, "L = 17: the ABI gives an empty row (the document l17 holds it)")
    add(L17[1:], "only_l16", "16 terms, the last one past the run in l16: no match")
    add([P, P], -1, "repeated term: P P in Q P P")
    add([P, Q, P], -1, "overlap: P Q P in P Q P Q P")
    add([P, Q, P, Q, P], "only_overlap", "the whole document")
    add([P, Q, P, Q, P, Q], "only_overlap", "one term longer than the document")
    add([Q, P, Q, P], "only_overlap", "overlapping starts, match at position 1")
    add([A, B, C_], "only_late", "a prefix match, a mismatch, then the real match later")
    add([A, B, C_], "only_prefix_only", "prefix matches only")
    add([A, B, C_], -1, "A B C over the corpus")
    for at in (62, 63, 64):
        add([C_, D], f"only_p{at}_2", f"two terms starting at stream position {at}")
        add([C_, D, E], f"only_p{at}_3", f"three terms starting at stream position {at}")
        add([C_, D, E], f"only_p{at}_2", f"three terms where only two stand at position {at}: no match")
    add([C_, D], -1, "C D over the corpus (ends on a chunk's last lane, straddles two chunks, starts the next)")
    add([C_, D, E], -1, "C D E over the corpus")
    add([D, E], "only_len63", "63 tokens: phrase on the last two")
    add([F, F, F], "only_len63", "a phrase of the filler")
    add([G, H], "only_len4097", "4097 tokens: the only occurrence at positions 4095 - 4096")
    add([G, H, E], "only_len10000", "10 000 tokens: the only occurrence at positions 4095 - 4097")
    add([G, H, E], "only_len4097", "4097 tokens: G H on the last tokens, E would be past the document")
    add([H, G], "only_len10000", "10 000 tokens: the only occurrence on the last two tokens")
    add([H, G], -1, "H G over the corpus")
    add([E, F, F, F, F, H], "only_len10000", "no match in 10 000 tokens (every chunk is read)")
    add([A, -1], -1, "an id of -1: empty row")
    add([N_TERMS, B], -1, "an id of n_terms: empty row")
    add([-1], -1, "L = 1 with an unknown id")
    add([], -1, "an empty phrase: empty row")
    add([], "odd", "an empty phrase with a candidate row")
    # phrases of the random documents: taken from a document (they match there) and drawn (most match somewhere by chance)
    rng = np.random.default_rng(7)
    lens = np.diff(c.tok_off)
    for d in np.nonzero(lens >= 6)[0][:40:8]:
        s = c.tok_ids[c.tok_off[d]:c.tok_off[d + 1]].tolist()
        add(s[2:4], -1, f"two terms of document {d}")
        add(s[1:4], "rnd", f"three terms of document {d}")
        add(s[-2:], "odd", f"the last two terms of document {d}")
    for i in range(6):
        add(rng.integers(0, N_RANDOM, 2).tolist(), ("rnd", -1, "odd")[i % 3], f"random pair {i}")
    return R


def cand_mask(c, r):
    """The mask row_cand value r stands for: None = every document."""
    if r == -1:
        return None
    return c.cands[r][1] if 0 <= r < len(c.cands) else np.zeros(c.n_docs, bool)


def random_rows(c, n, seed=5):
    """n rows: phrases of 1 .. 3 random terms, two terms taken from a document, planted phrases and invalid ones; any row_cand."""
    rng = np.random.default_rng(seed)
    fixed = [[A, B], [C_, D], [X, Y], [P, Q, P], [G, H], [], [A, -1], L17, [X], [A, B, C_]]
    lens = np.diff(c.tok_off)
    long = np.nonzero(lens >= 3)[0]
    rows = []
    for i in range(n):
        kind = i % 4
        if kind == 0:
            p = fixed[(i // 4) % len(fixed)]
        elif kind == 1 and len(long):
            d = int(long[rng.integers(0, len(long))])
            at = int(rng.integers(0, lens[d] - 1))
            p = c.tok_ids[c.tok_off[d] + at:c.tok_off[d] + at + 2].tolist()
        else:
            p = rng.integers(0, N_RANDOM, int(rng.integers(1, 4))).tolist()
        rows.append(RowCase(p, int(rng.integers(-1, 4)) if i % 5 else len(c.cands), f"random row {i}"))
    return rows


@lru_cache(maxsize=None)
def expected(N, empty_ends=False):
    """(cases, [bool [N]] the oracle's mask of each) of a corpus: computed once, shared by the tests, never changed."""
    c = corpus(N, empty_ends)
    cases = row_cases(c)
    want = [phrase_mask(c.tok_off, c.tok_ids, r.phrase, cand_mask(c, r.cand)) for r in cases]
    for w in want:
        w.setflags(write=False)
    return cases, want
