"""Document layouts for the K-split dense sweep (dense_ksplit_kernel, csrc/msr_dense_ks.hip).  TEST INFRASTRUCTURE ONLY.

The kernel keeps per-document maxima in an LDS ring (128 documents, 64 in the 128-query bf16 instance) and retires them in
aligned blocks of 32 documents, at most two blocks per 16-row unit.  Whether a corpus may take it is decided at bind time
(chunk_layout, csrc/msr_engine.hip).  This module holds

  * `bind_rule`: a Python restatement of that decision (the window rule, the one-group rule, and the walk of the kernel's
    own block bookkeeping that refuses a corpus whose retirement would lag a whole ring behind the rows);
  * `ring_walk`: a restatement of the kernel's bookkeeping alone -- which rows land in which ring slot, which block is
    retired when -- with the retirement policy as a parameter.  No arithmetic: it reports the documents that would come
    back with another document's rows, or without some of their own;
  * `CASES`: named layouts (doc_off only) at the edges of the rule and beyond them, each with the verdict it must get;
  * `build`: fills a layout with random unit rows and queries, one of them a scaled row of a chosen document;
  * `check_dense`: the project's dense parity check against oracle.dense_ref (shared with tests/test_gpu_parity.py).

Everything is deterministic from a seed and runs without a GPU."""
from dataclasses import dataclass, field

import numpy as np

DIM = 768
RING = 128              # MSR_WIDE_RING
RING64 = 64             # the 128-query bf16 instance
BLOCK = 32              # documents per retired block
UNIT = 16               # rows per unit
SPAN_MIN_ROWS = 256     # make_spans(n_cus, 256): the K-split kernels' spans


# ------------------------------------------------------------------------------------------------ the bind rule
def make_spans(doc_off, target, min_rows=SPAN_MIN_ROWS):
    """chunk_layout's make_spans: `target` spans of equal row count, cut at the first document starting at or after the cut."""
    off = np.asarray(doc_off, np.int64)
    n_docs, n_chunks = len(off) - 1, int(off[-1])
    if target * min_rows > n_chunks:
        target = max(1, n_chunks // min_rows)
    sp = [0]
    for s in range(1, target):
        d = min(int(np.searchsorted(off, n_chunks * s // target, side="left")), n_docs)
        if d > sp[-1]:
            sp.append(d)
    if sp[-1] != n_docs:
        sp.append(n_docs)
    return sp


def _last_doc_below(off, row):
    """Document of row `row` (the last document starting at or before it)."""
    return int(np.searchsorted(off, row, side="right")) - 1


def window_rule(doc_off):
    """-> (wide_ok, wide_ok64) by the window rule alone: the documents under two consecutive 16-row groups fit the ring
    with a block to spare (first to last document at most ring - 32 apart), and one group's rows span at most 32."""
    off = np.asarray(doc_off, np.int64)
    n_chunks = int(off[-1])
    ok, ok64 = True, True
    for u in range((n_chunks + UNIT - 1) // UNIT):
        dl = _last_doc_below(off, UNIT * u)
        dr = _last_doc_below(off, min(UNIT * (u + 2), n_chunks) - 1)
        dm = _last_doc_below(off, min(UNIT * (u + 1), n_chunks) - 1)
        if dr - dl + BLOCK > RING:
            ok = False
        if dr - dl + BLOCK > RING64:
            ok64 = False
        if dm - dl > BLOCK:
            ok = ok64 = False
    return ok, ok64


def retire_lag(doc_off, spans, retire=2):
    """The walk the bind makes: per span the kernel's next_b / next_end bookkeeping with `retire` blocks per unit at most
    (None: no limit).  -> the largest (document being folded) - (first document not yet retired) over all units."""
    off = np.asarray(doc_off, np.int64)
    worst = 0
    for d0, d1 in zip(spans[:-1], spans[1:]):
        c0, c1 = int(off[d0]), int(off[d1])
        nb = d0 & ~(BLOCK - 1)
        end = lambda b: int(off[min(b + BLOCK, d1)])
        while nb < d1 and end(nb) <= c0:                     # flush_done(c0): leading chunk-less blocks
            nb += BLOCK
        for g in range(c0 // UNIT, (c1 + UNIT - 1) // UNIT if c1 > c0 else c0 // UNIT):
            worst = max(worst, _last_doc_below(off, min(UNIT * g + UNIT, c1) - 1) - nb)
            n = 0
            while nb < d1 and end(nb) <= UNIT * g and (retire is None or n < retire):   # flush_step(16 g)
                nb += BLOCK
                n += 1
    return worst


def bind_rule(doc_off, n_cus=256, lag_walk=True):
    """The bind-time decision restated -> dict(wide_ok, wide_ok64, tiles_ok, n_spans).  lag_walk=False is the rule before
    the walk was added (windows only)."""
    off = np.asarray(doc_off, np.int64)
    spans = make_spans(off, n_cus)
    ok, ok64 = window_rule(off)
    if lag_walk and (ok or ok64):
        lag = retire_lag(off, spans, retire=2)
        ok = ok and lag < RING
        ok64 = ok64 and lag < RING64
    return dict(wide_ok=int(ok), wide_ok64=int(ok64), tiles_ok=int(np.diff(off).max(initial=0) <= 256), n_spans=len(spans) - 1)


# ------------------------------------------------------------------------------------------------ the ring bookkeeping
def ring_walk(doc_off, spans, ring=RING, retire=2):
    """What the kernel's ring reports, by bookkeeping alone.  Every wave folds unit g's rows into slot
    (document - dbase) & (ring - 1), then retires the blocks that were complete BEFORE unit g (rows_done = 16 g), at most
    `retire` of them (None: all); the pipelined instance does the same one barrier later, which changes no order between a
    fold and a retirement.  A retired block reports, for each of its documents, the rows its slot holds, and empties it.
    -> sorted documents whose reported rows are not exactly their own (mislabelled or lost)."""
    off = np.asarray(doc_off, np.int64)
    chunk_doc = np.repeat(np.arange(len(off) - 1), np.diff(off))
    wrong = []
    for d0, d1 in zip(spans[:-1], spans[1:]):
        c0, c1 = int(off[d0]), int(off[d1])
        dbase = d0 & ~(BLOCK - 1)
        slots = {}
        nb = dbase
        end = lambda b: int(off[min(b + BLOCK, d1)])

        def flush(b):
            for d in range(b, b + BLOCK):
                got = slots.pop((d - dbase) & (ring - 1), [])
                if d0 <= d < d1 and got != list(range(int(off[d]), int(off[d + 1]))):
                    wrong.append(d)

        while nb < d1 and end(nb) <= c0:
            flush(nb)
            nb += BLOCK
        g0 = c0 // UNIT
        g1 = (c1 + UNIT - 1) // UNIT if c1 > c0 else g0
        for g in range(g0, g1):
            for r in range(max(UNIT * g, c0), min(UNIT * g + UNIT, c1)):
                slots.setdefault((int(chunk_doc[r]) - dbase) & (ring - 1), []).append(r)
            n = 0
            while nb < d1 and end(nb) <= UNIT * g and (retire is None or n < retire):
                flush(nb)
                nb += BLOCK
                n += 1
        while nb < d1:                                       # flush_done(all rows)
            flush(nb)
            nb += BLOCK
    return sorted(wrong)


# ------------------------------------------------------------------------------------------------ layouts
def offsets(counts):
    off = np.zeros(len(counts) + 1, np.int64)
    off[1:] = np.cumsum(np.asarray(counts, np.int64))
    return off


def sustained(rows_per_doc, n_docs_with_rows, gap, repeats):
    """`repeats` x (n_docs_with_rows documents of rows_per_doc rows -- 16 rows in all -- then `gap` chunk-less documents)."""
    assert rows_per_doc * n_docs_with_rows == UNIT
    return ([rows_per_doc] * n_docs_with_rows + [0] * gap) * repeats


def _dense_tail(n=6):
    return [UNIT] * n                                        # 16-row documents: every later window spans 2 documents


def window_edge(span, lead):
    """Two consecutive groups whose documents span exactly `span` (>= 34): a 16-row document, then the second group spread
    over the last 33 documents of the span (one group spans 32, the most it may); `lead` chunk-less documents in front."""
    gap = span - 33                                          # chunk-less documents between the first group and the second
    second = [1] * 15 + [0] * 17 + [1]                       # 16 rows over 33 documents
    return [0] * lead + [UNIT] + [0] * gap + second + _dense_tail()


def ring64_edge(span, lead):
    """The same for the 64-document ring: the second group is 16 one-row documents ending `span` documents after the first."""
    return [0] * lead + [UNIT] + [0] * (span - 16) + [1] * 16 + _dense_tail()


def one_group_edge(span, lead):
    """One group whose 16 one-row documents span `span` (>= 31) documents, chunk-less ones between them."""
    grp = [1, 0] * 15 + [0] * (span - 30) + [1]
    return [0] * lead + grp + _dense_tail()


def _body(seed, n_docs=100):
    return np.random.default_rng(seed).integers(1, 6, size=n_docs).tolist()


@dataclass
class Case:
    name: str
    counts: list                       # chunks per document
    window: tuple                      # (wide_ok, wide_ok64) the window rule must give
    wide: tuple                        # (wide_ok, wide_ok64) the bind must give (window rule and the retirement walk)
    loses: bool = False                # the two-blocks-per-unit kernel would misreport documents if it ran on this layout
    family: str = ""
    shard: tuple = None                # (rank, world): the case is CorpusIndex.shard(rank, world) of `counts`
    doc_off: np.ndarray = field(default=None, repr=False)

    def __post_init__(self):
        self.doc_off = offsets(self.counts)


def _shard_counts(counts, rank, world):
    """CorpusIndex.shard_bounds restated (cuts balanced by chunk count, first document at or after the cut)."""
    off = offsets(counts)
    cuts = np.searchsorted(off, (off[-1] * np.arange(1, world)) // world, side="left")
    b = np.maximum.accumulate(np.concatenate([[0], np.minimum(cuts, len(counts)), [len(counts)]]))
    return b, list(counts[int(b[rank]):int(b[rank + 1])])


def _cases():
    Y, N = (1, 1), (0, 0)
    out = []
    add = lambda *a, **k: out.append(Case(*a, **k))
    # the window rule's edges; the first document at offset 0 and at offset 31 of its block of 32
    for lead in (0, 31):
        add(f"window96_lead{lead}", window_edge(96, lead), (1, 0), (1, 0), family="edge")
        add(f"window97_lead{lead}", window_edge(97, lead), (0, 0), (0, 0), loses=lead == 31, family="edge")
        add(f"ring64_span32_lead{lead}", ring64_edge(32, lead), Y, Y, family="edge")
        add(f"ring64_span33_lead{lead}", ring64_edge(33, lead), (1, 0), (1, 0), family="edge")
        add(f"group32_lead{lead}", one_group_edge(32, lead), (1, 0), (1, 0), family="edge")
        add(f"group33_lead{lead}", one_group_edge(33, lead), N, N, family="edge")
    # sustained sparse layouts: the window rule takes them all, the two-block retirement falls behind on some
    for rows, docs, gap, lost in ((16, 1, 64, False), (16, 1, 70, True), (16, 1, 80, True), (16, 1, 95, True),
                                  (1, 16, 48, False), (1, 16, 56, True), (1, 16, 64, True)):
        add(f"sustained_{docs}x{rows}_gap{gap}_x16", sustained(rows, docs, gap, 16), (1, 0), N if lost else (1, 0),
            loses=lost, family="sustained")
    add("sustained_1x16_gap80_x64", sustained(16, 1, 80, 64), (1, 0), N, loses=True, family="sustained")
    add("sustained_1x16_gap95_x64", sustained(16, 1, 95, 64), (1, 0), N, loses=True, family="sustained")
    # accepted sustained layouts large enough for span cuts inside the pattern (1 024 and 3 072 rows; the second cuts
    # groups and blocks at odd places: 5 + 11 rows per pair of documents)
    add("sustained_1x16_gap64_x64", sustained(16, 1, 64, 64), (1, 0), (1, 0), family="sustained")
    add("sustained_5and11_gap40_x192", ([5, 11] + [0] * 40) * 192, (1, 0), (1, 0), family="sustained")
    # leading and trailing runs of chunk-less documents
    for run in (1, 31, 32, 33, 95, 96, 97, 200):
        add(f"leading_run{run}", [0] * run + _body(run), Y, Y, family="runs")
        add(f"trailing_run{run}", _body(100 + run) + [0] * run, Y, Y, family="runs")
    # a partial last block of 32 documents and a partial last group of 16 rows
    for docs_mod, rows_mod in ((1, 1), (31, 15), (1, 15), (31, 1)):
        c = _body(7 * docs_mod + rows_mod, 64 + docs_mod)
        c[-1] += (rows_mod - sum(c)) % UNIT
        assert len(c) % BLOCK == docs_mod and sum(c) % UNIT == rows_mod
        add(f"partial_docs{docs_mod}_rows{rows_mod}", c, Y, Y, family="runs")
    # one document owning every row; a document of 300 rows in the middle of a sparse pattern
    add("one_document_200_rows", [200], Y, Y, family="owner")
    add("one_owner_among_chunkless", [0] * 40 + [200] + [0] * 50, Y, Y, family="owner")
    # (300 rows shift the pattern behind it by 12 rows: every later group holds rows of two documents 31 apart)
    add("doc300_inside_sparse", sustained(16, 1, 30, 8) + [300] + [0] * 30 + sustained(16, 1, 30, 8), (1, 0), (1, 0),
        family="owner")
    # shards of the 95-gap layout: shard 0 ends right after a document with rows, shard 1 begins with the run behind it
    for r in range(2):
        b, c = _shard_counts(sustained(16, 1, 95, 64), r, 2)
        add(f"shard{r}of2_gap95_x64", c, (1, 0), N, loses=True, family="shards", shard=(r, 2))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def random_sustained(rng):
    """One layout of the sustained family: a 16-row unit (1, 2, 4, 8 or 16 documents) and a chunk-less gap, 16 repeats, the
    gap drawn so that the window rule takes most of them and the retirement walk about two thirds of those."""
    docs = int(rng.choice([1, 2, 4, 8, 16]))
    gap = int(rng.integers(0, 97 - docs))
    jitter = int(rng.integers(0, 9))                         # every repeat's gap shortened by 0 .. jitter documents
    counts = []
    for _ in range(16):
        counts += [UNIT // docs] * docs + [0] * max(0, gap - int(rng.integers(0, jitter + 1)))
    return [0] * int(rng.integers(0, 40)) + counts


# ------------------------------------------------------------------------------------------------ corpora
@dataclass
class Corpus:
    case: Case
    doc_off: np.ndarray                # int64 [n_docs + 1]
    emb: np.ndarray                    # float32 [n_chunks, 768], unit rows
    q: np.ndarray                      # float32 [128, 768]; q[0] is 3 x the first row of document `planted`
    planted: int
    with_rows: np.ndarray              # documents that have chunks, ascending


def planted_document(case):
    """A document the two-block kernel would lose (the first one with rows among the misreported ones); where it loses
    none, the last document with rows -- the one whose ring slot is written latest."""
    off = case.doc_off
    has = np.diff(off) > 0
    if case.loses:
        for d in ring_walk(off, make_spans(off, 256), RING, retire=2):
            if has[d]:
                return d
    return int(np.nonzero(has)[0][-1])


def build(case, seed=0, n_queries=128):
    rng = np.random.default_rng([seed, len(case.counts), int(case.doc_off[-1])])
    emb = rng.standard_normal((int(case.doc_off[-1]), DIM)).astype(np.float32)
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)
    q = (rng.standard_normal((n_queries, DIM)) * rng.uniform(0.5, 9)).astype(np.float32)
    d = planted_document(case)
    q[0] = emb[case.doc_off[d]] * 3.0
    return Corpus(case, case.doc_off, emb, q, d, np.nonzero(np.diff(case.doc_off) > 0)[0])


# ------------------------------------------------------------------------------------------------ the parity check
def check_dense(mods, eng, doc_off, emb, q, k, mc, got):
    """HIP dense top-k `got` = (doc, score, chunk, n) against oracle.dense_ref: scores within 1e-5, set differences only among
    scores within 2e-5 of the k-th, exact ties by ascending document, the arg-max row inside the document and within 2e-5.
    mods: dict with the oracle modules `dense_ref` and `rerank_ref`."""
    doc, score, chunk, n = [x.cpu().numpy() for x in got]
    for i in range(q.shape[0]):
        best, arg = mods["dense_ref"].doc_scores(emb, doc_off, q[i], mc)
        oi, os_, oa = mods["dense_ref"].quick_search(emb, doc_off, q[i], k, mc)
        assert n[i] == len(oi)
        np.testing.assert_allclose(score[i, :n[i]], os_, rtol=0, atol=1e-5)        # north_star: 1e-5 fp32
        np.testing.assert_allclose(score[i, :n[i]], best[doc[i, :n[i]]], rtol=0, atol=1e-5)
        assert np.all(np.diff(score[i, :n[i]]) <= 0)
        # same documents, except for swaps among scores closer than the tolerance
        diff = set(doc[i, :n[i]].tolist()) ^ set(oi.tolist())
        for d in diff:
            assert abs(best[d] - os_[-1]) <= 2e-5
        # ties broken by ascending index where the scores are exactly equal
        for j in range(1, n[i]):
            if score[i, j] == score[i, j - 1]:
                assert doc[i, j] > doc[i, j - 1]
        # arg-max chunk row
        for j in range(n[i]):
            d = doc[i, j]
            c = chunk[i, j]
            lo, hi = doc_off[d], doc_off[d + 1]
            if mc:
                hi = min(hi, lo + mc)
            assert lo <= c < hi
            cos_c = float(mods["rerank_ref"].cosine_f32(q[i], emb[c:c + 1])[0])
            assert abs(cos_c - best[d]) <= 2e-5
