"""Cases for the index-maintenance kernels (csrc/msr_build.hip, msr_merge.hip, msr_compact.hip and the scan they share) and
a plain numpy reference of the build.  tests/test_index_cases.py checks the cases and the reference on the CPU;
tests/test_gpu_index_edges.py runs the same cases through the kernels.

reference  ref_build: key = term * n_docs + document per token, np.unique with counts, bincount + cumsum.  Nothing of
           msretr.index_build is used.
build      every case is CONSTRUCTED to hit an edge of the kernels exactly and records what it claims (BuildCase): the
           chunks of every document, the postings before and after the chunk merge, the radix passes.  The claims come from
           the construction's own bookkeeping, never from running a builder; test_index_cases.py recomputes them.
merge /    the shapes of the index update and removal tests (side / maps / table), which those tests import from here.
compact
The kernel constants the edges depend on are read from the sources (constants()): a changed constant fails the CPU tests
instead of quietly moving the kernels' edges away from the cases."""
import os
import re
from dataclasses import dataclass, field

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "modern-search-engines-project_amd", "csrc")


def constants():
    """{'CH', 'RB', 'MSR_SCAN_BLOCK', 'MERGE_TILE', 'COMPACT_TILE'} parsed from the kernel sources."""
    def src(name):
        with open(os.path.join(CSRC, name), encoding="utf-8") as f:
            return f.read()

    def const(text, name):
        return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))
    build, merge, compact, internal = src("msr_build.hip"), src("msr_merge.hip"), src("msr_compact.hip"), src("msr_internal.h")
    assert re.search(r"constexpr int SB = MSR_SCAN_BLOCK;", build)
    assert re.search(r"constexpr int TILE = MT \* ITEMS;", merge) and re.search(r"constexpr int TILE = 4 \* QUADS;", compact)
    assert re.search(r"constexpr int QUADS = MT \* ROUNDS;", compact)
    return dict(CH=const(build, "CH"), RB=const(build, "RB"), MSR_SCAN_BLOCK=const(internal, "MSR_SCAN_BLOCK"),
                MERGE_TILE=const(merge, "MT") * const(merge, "ITEMS"),
                COMPACT_TILE=4 * const(compact, "MT") * const(compact, "ROUNDS"))


CH = 4096                # tokens per chunk of unique_kernel            } asserted against the sources by
RB = 4096                # entries per radix block of scatter_kernel     } test_index_cases.py
SCAN_BLOCK = 4096        # MSR_SCAN_BLOCK                               }
MERGE_TILE = 2048
COMPACT_TILE = 2048


# ---------------------------------------------------------------------------------------------------------------- reference
def ref_build(tok_off, tok_ids, n_terms):
    """(term_off int64 [n_terms + 1], post_doc int32, post_tf int32) of the documents tok_ids[tok_off[i]:tok_off[i + 1]]:
    CSR by term, documents ascending inside a term, tf = occurrences."""
    tok_off = np.asarray(tok_off, np.int64)
    n_docs = len(tok_off) - 1
    doc = np.repeat(np.arange(n_docs, dtype=np.int64), np.diff(tok_off))
    key = np.asarray(tok_ids, np.int64) * max(n_docs, 1) + doc
    uniq, tf = np.unique(key, return_counts=True)
    term_off = np.zeros(n_terms + 1, np.int64)
    term_off[1:] = np.cumsum(np.bincount(uniq // max(n_docs, 1), minlength=n_terms))
    return term_off, (uniq % max(n_docs, 1)).astype(np.int32), tf.astype(np.int32)


def radix_passes(n_terms):
    """8-bit passes over ceil(log2(n_terms)) bits."""
    return (int(n_terms - 1).bit_length() + 7) // 8


# ---------------------------------------------------------------------------------------------------------------- build cases
@dataclass
class BuildCase:
    name: str
    tok_off: np.ndarray          # int64 [n_docs + 1]
    tok_ids: np.ndarray          # int32
    n_terms: int
    chunks: np.ndarray           # claimed: chunks of every document
    p_pre: int                   # claimed: (chunk, term) pairs = entries the radix sort moves
    p_post: int                  # claimed: (document, term) pairs = postings
    passes: int                  # claimed: radix passes
    notes: dict = field(default_factory=dict)

    @property
    def n_docs(self):
        return len(self.tok_off) - 1

    @property
    def split(self):
        return bool((self.chunks > 1).any())


class _Corpus:
    """Documents given chunk by chunk, each chunk as (its distinct terms, its length); counts the claims as it goes."""

    def __init__(self, rng):
        self.rng, self.docs, self.chunks, self.p_pre, self.p_post = rng, [], [], 0, 0

    def add(self, *chunks):
        """One document; every chunk but the last must be CH tokens long."""
        toks, seen = [], set()
        for j, (terms, length) in enumerate(chunks):
            terms = np.asarray(terms, np.int64)
            assert len(set(terms.tolist())) == len(terms) and 1 <= len(terms) <= length <= CH
            assert length == CH or j == len(chunks) - 1
            t = np.concatenate([terms, terms[self.rng.integers(0, len(terms), length - len(terms))]])
            toks.append(self.rng.permutation(t))
            self.p_pre += len(terms)
            seen.update(terms.tolist())
        self.p_post += len(seen)
        self.chunks.append(len(chunks))
        self.docs.append(np.concatenate(toks))
        return len(self.docs) - 1

    def case(self, name, n_terms, **notes):
        off = np.zeros(len(self.docs) + 1, np.int64)
        off[1:] = np.cumsum([len(d) for d in self.docs])
        return BuildCase(name, off, np.concatenate(self.docs).astype(np.int32), n_terms, np.array(self.chunks), self.p_pre,
                         self.p_post, radix_passes(n_terms), notes)


def _with(rng, n_terms, k, *must):
    """k distinct terms that include `must`."""
    must = list(dict.fromkeys(must))
    rest = rng.choice(n_terms, k + len(must), replace=False)
    rest = rest[~np.isin(rest, must)][:k - len(must)]
    return np.concatenate([np.array(must, np.int64), rest])


CHUNK_EDGE_LENGTHS = (1, 63, 64, 65, 4095, 4096, 4097, 8192, 8193, 12289)


def chunk_edge_corpus():
    """Documents of the lengths where unique_kernel pads, fills or splits a chunk, among short ones; term 0 in every document;
    a 12289-token document of one term (four chunk entries merged into tf 12289); a 4096-token document of 4096 distinct
    terms; the last term id in several documents."""
    rng = np.random.default_rng(401)
    V = 6000
    c = _Corpus(rng)
    notes = {}

    def shorts(n):
        for _ in range(n):
            L = int(rng.integers(1, 40))
            c.add((_with(rng, V, int(rng.integers(1, L + 1)), 0), L))
    shorts(40)
    for L in CHUNK_EDGE_LENGTHS:
        spec, left = [], L
        while left > 0:
            n = min(CH, left)
            k = int(rng.integers(1, min(n, 700) + 1))
            spec.append((_with(rng, V, k, 0) if not spec else _with(rng, V, k, int(spec[0][0][-1])), n))
            left -= n
        if L == 4097:                                   # the trailing chunk: one token, a term of the first chunk
            spec[-1] = (spec[0][0][1:2] if len(spec[0][0]) > 1 else spec[0][0][:1], 1)
        notes[f"len{L}"] = c.add(*spec)
        shorts(7)
    notes["one_term"] = c.add(([0], CH), ([0], CH), ([0], CH), ([0], 1))
    shorts(5)
    notes["all_distinct"] = c.add((_with(rng, V, CH, 0, V - 1), CH))
    shorts(5)
    c.add((_with(rng, V, 3000, 0, V - 1), CH), (_with(rng, V, 3000, V - 1), CH), (_with(rng, V, 17, V - 1, 1), 17))
    shorts(30)
    c.add(([0, V - 1], 2))
    return c.case("chunk_edges", V, **notes)


RADIX_EDGE_P = (1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 2 * 4096 - 1, 2 * 4096 + 1, 37 * 4096 + 5)


def radix_edge_corpus(P, split):
    """Exactly P postings from documents of distinct tokens over 300 terms (two radix passes, every digit value crowded: the
    stable ranking of scatter_kernel crosses lanes, 64-lane rounds, waves and blocks).  split: one 4097-token document in
    the middle whose trailing one-token chunk repeats a term of its first chunk, so the sort moves P + 1 entries and the
    chunk merge drops one."""
    rng = np.random.default_rng(500 + P + (7 if split else 0))
    V = 300
    c = _Corpus(rng)
    s = min(P, 30) if split else 0
    lens, left = [], P - s
    while left > 0:
        lens.append(min(left, int(rng.integers(1, 41))))
        left -= lens[-1]
    for i, L in enumerate(lens):
        if split and i == len(lens) // 2:
            terms = _with(rng, V, s)
            c.add((terms, CH), (terms[:1], 1))
        c.add((_with(rng, V, L), L))
    if split and not lens:
        terms = _with(rng, V, s)
        c.add((terms, CH), (terms[:1], 1))
    case = c.case(f"radix_P{P}_{'split' if split else 'whole'}", V)
    assert case.p_post == P and case.p_pre == P + (1 if split else 0)
    return case


PASS_COUNT_TERMS = (1, 2, 256, 257, 65536, 65537, 1 << 24, (1 << 24) + 1)


def pass_count_corpus(n_terms):
    """A few thousand postings over a sparse vocabulary of n_terms: the lowest ids, the highest ids, and ids that differ only in
    the byte of the last radix pass."""
    rng = np.random.default_rng(600 + n_terms % 1000)
    passes = radix_passes(n_terms)
    shift = 8 * max(passes - 1, 0)
    pool = set(range(min(n_terms, 40))) | set(range(max(n_terms - 40, 0), n_terms))
    top = (n_terms - 1) >> shift
    for b in sorted(set(np.linspace(0, top, min(top + 1, 48)).astype(int).tolist())):
        for low in (0, 5, 0xAB, 0x1234 & ((1 << shift) - 1)):
            if ((b << shift) | low) < n_terms:
                pool.add((b << shift) | low)
    pool = np.array(sorted(pool), np.int64)
    c = _Corpus(rng)
    for _ in range(1500):
        k = int(rng.integers(1, min(len(pool), 4) + 1))
        c.add((rng.choice(pool, k, replace=False), k + int(rng.integers(0, 3))))
    c.add((pool[[0, -1]] if len(pool) > 1 else pool[:1], 2))
    return c.case(f"passes_V{n_terms}", n_terms, pool=pool)


SCALE_V = 65521                                            # prime: (start + stride * j) % V is injective in j < V


def scale_corpus(n_docs=95_000, doc_len=180, long_len=9000, long_mod=5000):
    """More than MSR_SCAN_BLOCK^2 postings after the chunk merge and one long document, so that the keep-flag scan inside
    msr_build_postings runs at three levels.  Document d = (start_d + stride_d * j) % SCALE_V for j < doc_len: distinct
    tokens, so every short document gives doc_len postings; the long one = (j + 11) % long_mod for j < long_len: its chunks
    hold distinct tokens (CH <= long_mod), its postings are long_mod."""
    assert doc_len < SCALE_V and CH <= long_mod < SCALE_V and long_mod < long_len
    rng = np.random.default_rng(701)
    start = rng.integers(0, SCALE_V, n_docs)[:, None]
    stride = rng.integers(1, SCALE_V, n_docs)[:, None]
    body = ((start + stride * np.arange(doc_len)[None, :]) % SCALE_V).astype(np.int32)
    long_doc = ((np.arange(long_len) + 11) % long_mod).astype(np.int32)
    at = n_docs // 3
    tok = np.concatenate([body[:at].ravel(), long_doc, body[at:].ravel()])
    lens = np.full(n_docs + 1, doc_len, np.int64)
    lens[at] = long_len
    off = np.zeros(n_docs + 2, np.int64)
    off[1:] = np.cumsum(lens)
    chunks = np.ones(n_docs + 1, np.int64)
    chunks[at] = -(-long_len // CH)
    return BuildCase("scale", off, tok, SCALE_V, chunks, n_docs * doc_len + long_len, n_docs * doc_len + long_mod,
                     radix_passes(SCALE_V), dict(long_doc=at))


def small_build_cases():
    """Every build case but the scale corpus, as (name, constructor)."""
    out = [("chunk_edges", chunk_edge_corpus)]
    for P in RADIX_EDGE_P:
        for split in (False, True):
            out.append((f"radix_P{P}_{'split' if split else 'whole'}", lambda P=P, split=split: radix_edge_corpus(P, split)))
    for V in PASS_COUNT_TERMS:
        out.append((f"passes_V{V}", lambda V=V: pass_count_corpus(V)))
    return out


# ---------------------------------------------------------------------------------------------------------------- merge / compact shapes
def side(rng, n_docs, n_terms, n_post, head=0, first_term=0):
    """CSR of exactly n_post postings over [0, n_docs) x [first_term, n_terms) (+ a head term 0 holding the first `head`
    documents), documents ascending inside a term."""
    span = (n_terms - first_term) * n_docs
    keys = np.unique(rng.integers(0, span, int(n_post * 1.3) + 16))
    keys = np.sort(rng.choice(keys, min(n_post, len(keys)), replace=False))
    term = keys // n_docs + first_term
    doc = keys % n_docs
    if head:
        keep = term != 0
        term = np.concatenate([np.zeros(head, np.int64), term[keep]])
        doc = np.concatenate([np.arange(head), doc[keep]])
    off = np.zeros(n_terms + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(term, minlength=n_terms))
    tf = rng.integers(1, 50, len(doc))
    return off, doc.astype(np.int32), tf.astype(np.int32)


def maps(rng, na, nb, pattern):
    if pattern == "appended":
        return None, np.arange(na, na + nb, dtype=np.int32)
    b = np.sort(rng.choice(na + nb, nb, replace=False)).astype(np.int32)
    a = np.setdiff1d(np.arange(na + nb), b).astype(np.int32)
    return a, b


def table(rng, n_docs, n_terms, n_post, head=0, empty_tail=0):
    """CSR of n_post postings over [0, n_docs) x [0, n_terms) (+ a head term 0 holding the first `head` documents, + the
    last `empty_tail` terms without postings), documents ascending inside a term."""
    live = n_terms - empty_tail
    keys = np.unique(rng.integers(0, live * n_docs, int(n_post * 1.3) + 16))
    keys = np.sort(rng.choice(keys, min(n_post, len(keys)), replace=False))
    term, doc = keys // n_docs, keys % n_docs
    if head:
        keep = term != 0
        term = np.concatenate([np.zeros(head, np.int64), term[keep]])
        doc = np.concatenate([np.arange(head), doc[keep]])
    off = np.zeros(n_terms + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(term, minlength=n_terms))
    return off, doc.astype(np.int32), rng.integers(1, 50, len(doc)).astype(np.int32)


MERGE_EDGE_P = tuple(k * MERGE_TILE + d for k, d in ((1, -1), (1, 0), (1, 1), (2, -1), (2, 0), (2, 1), (37, 5)))
COMPACT_EDGE_P = tuple(k * COMPACT_TILE + d for k, d in ((1, -1), (1, 0), (1, 1), (2, -1), (2, 3), (37, 5)))


def merge_edge_case(P, pattern):
    """The inputs of test_gpu_index_update.test_merge_tile_edges: (a, a_map, b, b_map, n_terms, n_docs, a_docs)."""
    rng = np.random.default_rng(P)
    na, nb, V = 3000, 400, 1200
    pb = P // 5
    a, b = side(rng, na, V, P - pb), side(rng, nb, V, pb)
    assert int(a[0][-1]) + int(b[0][-1]) == P
    a_map, b_map = maps(rng, na, nb, pattern)
    return a, a_map, b, b_map, V, na + nb, na


def merge_head_case(pattern):
    """A head term that spans many tiles on both sides, terms on one side only and new terms (the shape of
    test_merge_head_term_and_one_sided_terms at a tenth of its size)."""
    rng = np.random.default_rng(31 if pattern == "appended" else 32)
    na, nb, V = 105_000, 1200, 3000
    a = side(rng, na, V, 40_000, head=na)
    b = side(rng, nb, V + 200, 6000, head=nb)
    keep = np.ones(len(b[1]), bool)
    keep[b[0][1]:b[0][100]] = False
    cnt = np.diff(b[0]); cnt[1:100] = 0
    b = (np.concatenate([[0], np.cumsum(cnt)]), b[1][keep], b[2][keep])
    a_map, b_map = maps(rng, na, nb, pattern)
    return a, a_map, b, b_map, V + 300, na + nb, na


def merge_one_posting_case():
    """Mostly one-posting terms on side A, new terms only on side B."""
    rng = np.random.default_rng(37)
    na, V = 5000, 200_000
    a = side(rng, na, V, 150_000)
    b = side(rng, 300, V + 50_000, 40_000, first_term=V)
    a_map, b_map = maps(rng, na, 300, "interleaved")
    return a, a_map, b, b_map, V + 50_000, na + 300, na
