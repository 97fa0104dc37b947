"""Inputs for the BM25 span-width tests (test_bm25_span_cases.py on the CPU, test_gpu_bm25_spans.py on the GPU).  Pure numpy.

The scoring kernel gives one wave a span of tpw = 1, 2, 4 or 8 consecutive 1024-document tiles; the number of queries in a call
picks tpw (split_rule restates the library's rule; the GPU test trusts the library's export, not this).  The corpus below has
61 tiles, the last one partial, and posting lists on every boundary the kernel and the select behind it distinguish: list
classes (read whole / probed / skip table), the per-tile chunk loop (64, 65, 128, 129, 384, 385 postings in one tile), tile
and span edges, empty spans, looked-up negative terms, scores far below the select's window."""
import math

import numpy as np

TILE = 1024
N_DOCS = 60 * TILE + 517                                      # 61 tiles, the last one partial
HEAVY_DF = 2048                                               # MSR_BM25_HEAVY_DF: lists at least this long get a skip-table row
MAX_DENSE = 64                                                # MSR_BM25_MAX_DENSE: negative lists with a dense table
SPAN8 = 8 * TILE

# queries in the call -> (tiles per wave, spans, tiles in the last span, select workgroups per query, segments per workgroup)
WIDTH_CASES = {
    16: (1, 61, 1, 61, 1),
    100: (1, 61, 1, 20, 4),                                   # select parts 16..19 own no segment
    255: (1, 61, 1, 8, 8),                                    # the last part owns 5 segments
    265: (2, 31, 1, 7, 5),                                    # the last part owns 1 segment
    512: (4, 16, 1, 4, 4),
    1023: (4, 16, 1, 2, 8),
    1024: (8, 8, 5, 2, 4),                                    # the last span is short and its tile count odd
}
SETTINGS = [(1000, 0.0), (10, 0.0), (1000, 0.75), (1000, -0.5), (100, -100.0)]      # (k, min_score)
TILE_COUNTS = (64, 65, 128, 129, 384, 385)                    # one prefetched chunk / two / + one streaming round / one more
TILE_POS = {"first": 0, "mid": 3, "last": 7}                  # position of the filled tile inside its span of 8


def split_rule(n_tiles, nq):
    """The library's rule (msr_bm25_split) restated: -> (tiles per wave, spans)."""
    tpw = 8
    while tpw > 1 and nq * ((n_tiles + tpw - 1) // tpw) < 8192:
        tpw >>= 1
    return tpw, (n_tiles + tpw - 1) // tpw


def select_parts(n_seg, nq):
    """The list select's split (select_impl / part_segments) restated: -> (workgroups per query, segments per workgroup)."""
    parts = max(1, min(n_seg, max(1, 2048 // nq)))
    return parts, (n_seg + parts - 1) // parts


def build_corpus(seed=77):
    """-> (z, T): z the index arrays oracle/bm25_ref and CorpusIndex take; T maps a list's name to its term id (or to a list
    of ids)."""
    rng = np.random.default_rng(seed)
    N = N_DOCS
    lists, idf, T = [], [], {}

    def add(name, docs, value):
        docs = np.unique(np.asarray(docs, np.int64))
        assert len(docs) and docs[0] >= 0 and docs[-1] < N
        lists.append(docs.astype(np.int32)); idf.append(value)
        tid = len(lists) - 1
        if name.endswith("[]"):
            T.setdefault(name[:-2], []).append(tid)
        else:
            assert name not in T
            T[name] = tid
        return tid

    bern = lambda p: np.nonzero(rng.random(N) < p)[0]
    pick = lambda n, lo=0, hi=N: lo + rng.choice(hi - lo, size=n, replace=False)
    for _ in range(70):
        add("neg[]", bern(0.6), -rng.uniform(0.05, 0.9))     # long, idf < 0: 64 get a dense table, 6 are streamed
    add("zero", bern(0.7), 0.0)                               # long, idf exactly 0
    add("pos_long", bern(0.55), 0.3)                          # long, idf > 0
    for n in (1, 63, 64, 65, 2047, 2048, 2049, 9000):         # whole-list lengths on every class boundary
        add("len_%d" % n, pick(n), rng.uniform(0.5, 3.0))
    # exactly c postings in single tiles, at the first / a middle / the last tile of a span of 8: medium lists (probed), and
    # the same with 1000 postings more far behind them (skip table)
    for pos, off in TILE_POS.items():
        docs = np.concatenate([pick(c, (8 * s + off) * TILE, (8 * s + off + 1) * TILE) for s, c in enumerate(TILE_COUNTS)])
        add("tile_med_" + pos, docs, rng.uniform(0.5, 3.0))
        docs = np.concatenate([pick(c, (8 * s + off) * TILE, (8 * s + off + 1) * TILE) for s, c in enumerate(TILE_COUNTS)])
        add("tile_heavy_" + pos, np.concatenate([docs, pick(1000, 48 * TILE, N)]), rng.uniform(0.5, 3.0))
    edges = [0, N - 1] + [t * TILE - 1 for t in range(1, 61)] + [t * TILE for t in range(1, 61)]
    add("edges", edges, 1.7)                                  # both sides of every tile edge, document 0 and N - 1
    add("straddle_8192", np.arange(8192 - 40, 8192 + 40), 2.1)    # a span-of-8, -4, -2 and tile edge at once
    add("straddle_2048", np.arange(2048 - 40, 2048 + 40), 1.3)    # a tile edge inside a span of 4 and 8, a span edge at 2
    add("one_tile", pick(300, 37 * TILE, 38 * TILE), 2.4)     # medium, entirely inside tile 37
    # 8 postings per tile, the last one on the tile's last document: 488 postings, probe chunks of ceil(488 / 64) = 8 postings
    # that end exactly on the tile (and so on every span) edges; the last three of the 64 probes are clamped
    docs = []
    for t in range(61):
        hi = min((t + 1) * TILE, N)
        docs += list(pick(7, t * TILE, hi - 1)) + [hi - 1]
    add("probe_chunks", docs, 0.9)
    add("heavy_blocks", np.concatenate([np.arange(5000, 6500), np.arange(50000, 51500)]), 1.1)   # whole empty spans
    add("heavy_dense", np.concatenate([np.arange(t * TILE, min((t + 1) * TILE, N)) for t in (20, 22, 59, 60)]), 0.8)
    add("short_neg", pick(30), -0.4)                          # short, idf < 0: streamed, no table
    add("strong", pick(12), 6.0)                              # the strongest term
    add("tiny_a", bern(0.75), 6e-7)                           # idf 1e-7 of the strongest
    add("tiny_all", np.arange(N), 1.8e-8)                     # idf 3e-9 of the strongest, in every document
    for _ in range(8):
        add("med[]", bern(0.01), rng.uniform(0.5, 3.0))      # ~600 postings: probed
    for _ in range(9):
        add("short[]", pick(30), rng.uniform(1.0, 4.0))
    for _ in range(4):
        add("hv[]", bern(0.08), rng.uniform(0.5, 2.5))       # ~5000 postings: skip table

    term_off = np.zeros(len(lists) + 1, np.int64); term_off[1:] = np.cumsum([len(x) for x in lists])
    post_doc = np.concatenate(lists)
    post_tf = rng.integers(1, 6, size=len(post_doc)).astype(np.int32)
    doc_len = rng.integers(5, 900, size=N).astype(np.int32)
    z = dict(doc_ids=np.arange(N, dtype=np.int64) * 2 + 1, doc_len=doc_len, term_off=term_off, post_doc=post_doc,
             post_tf=post_tf, idf=np.asarray(idf, np.float32), avgdl=float(np.float32(doc_len.mean())))
    # the negative lists WITHOUT a table: all but the MAX_DENSE longest (the engine's stable sort by length, descending)
    neg = T["neg"]
    order = sorted(neg, key=lambda t: -(term_off[t + 1] - term_off[t]))
    T["neg_untabled"] = sorted(order[MAX_DENSE:])
    T["neg_tabled"] = sorted(order[:MAX_DENSE])
    return z, T


def build_queries(z, T, seed=78):
    """Some 40 distinct queries (lists of term ids, repeats allowed) -> (queries, names)."""
    rng = np.random.default_rng(seed)
    V = len(z["idf"])
    neg, med, short, hv, unt = T["neg_tabled"], T["med"], T["short"], T["hv"], T["neg_untabled"]
    tiles = [T["tile_%s_%s" % (c, p)] for c in ("med", "heavy") for p in TILE_POS]
    Q = [
        ("neg_first", [neg[3], med[0], short[0]]),
        ("neg_last", [med[0], short[0], neg[3]]),
        ("neg_between", [med[0], neg[3], short[0], neg[5], short[1]]),
        ("neg_repeated", [neg[3], neg[3], med[0]]),
        ("neg_alone", [neg[3]]),
        ("neg_alone3", [neg[3], neg[5], neg[7]]),
        ("untabled", unt + [med[0]]),
        ("untabled_alone", list(unt)),
        ("zero_first", [T["zero"], neg[3]]),
        ("zero_between", [neg[3], T["zero"], med[0]]),
        ("pos_long", [T["pos_long"], neg[3], med[0]]),
        ("short_neg", [T["short_neg"], short[0]]),
        ("short_neg_lookup", [T["short_neg"], neg[3]]),
        ("short_neg_alone", [T["short_neg"]]),
        ("beyond_prefetch", [med[0], neg[1], med[1], neg[2], med[2], neg[3], med[3], neg[4], med[4], neg[5], med[5], neg[6],
                             short[0], neg[7]]),
        ("mix50", [int(t) for t in rng.permutation(V)[:50]]),
        ("mix64", [int(t) for t in rng.permutation(V)[:64]]),
        ("lookups_before_term_63", neg[:62] + [short[7], short[8]]),      # first touches at the LAST of 64 term positions
        ("no_neg", [short[0], short[1], short[2]]),
        ("unknown_ids", [V + 110, -3, neg[3], med[0]]),
        ("len_1", [T["len_1"]]),
        ("len_64", [T["len_63"], T["len_64"], T["len_65"]]),
        ("len_2048", [T["len_2047"], T["len_2048"], T["len_2049"]]),
        ("len_9000", [T["len_9000"], neg[0]]),
        ("edges", [T["edges"]]),
        ("edges_combined", [T["edges"], T["straddle_8192"], neg[10], T["straddle_2048"], T["len_2049"], T["probe_chunks"]]),
        ("straddle_8192", [T["straddle_8192"]]),
        ("straddle_2048", [T["straddle_2048"], hv[0]]),
        ("one_tile", [T["one_tile"]]),                        # every other span emits length 0
        ("one_tile_lookups", [neg[4], T["one_tile"], neg[9]]),
        ("probe_chunks", [T["probe_chunks"]]),
        ("tiles_med_first", tiles[:3] + tiles[3:]),           # the medium lists among the four prefetched terms
        ("tiles_heavy_first", tiles[3:] + [neg[8]] + tiles[:3]),
        ("tiles_behind_prefetch", [short[3], short[4], short[5], short[6]] + tiles),
        ("heavy_blocks", [T["heavy_blocks"]]),
        ("heavy_dense", [T["heavy_dense"], neg[2], T["heavy_blocks"]]),
        ("hv_pair", [hv[1], neg[11], hv[2], hv[2]]),
        ("strong_tiny", [T["strong"], T["tiny_a"]]),
        ("strong_tiny_all", [T["strong"], T["tiny_a"], med[2], T["tiny_all"]]),
        ("tiny_a", [T["tiny_a"]]),
        ("tiny_all", [T["tiny_all"]]),
        ("strong_x40", [T["strong"]] * 40 + [T["tiny_all"]]),
        ("empty", []),
    ]
    return [q for _, q in Q], [n for n, _ in Q]


def fill(n_distinct, nq, start=0):
    """Row r of a call of nq queries runs distinct query fill(...)[r]: the distinct queries repeated with a stride coprime to
    their number, so that a query sits at many different positions of the call.  A call of fewer rows than there are distinct
    queries is repeated with start = nq, 2 nq, ... until every query has run (calls_for)."""
    stride = next(s for s in range(7, 7 + n_distinct) if math.gcd(s, n_distinct) == 1)
    return ((start + np.arange(nq, dtype=np.int64)) * stride) % n_distinct


def calls_for(n_distinct, nq):
    """The `start` values of the calls of nq rows that together run every distinct query."""
    return list(range(0, max(n_distinct, 1), nq)) if nq < n_distinct else [0]


def within_masks(n_docs=N_DOCS):
    """The document sets of the restricted calls: name -> bool [n_docs] (None: unrestricted)."""
    m = lambda: np.zeros(n_docs, bool)
    one, other, block, tail = m(), m(), m(), m()
    one[8192] = True
    other[::2] = True
    block[8000:8400] = True                                   # crosses a tile edge and a span edge of every width
    tail[(n_docs // 32) * 32:] = True                         # the last, partial 32-bit word
    return {"none": None, "empty": m(), "one": one, "every_other": other, "block": block, "tail_word": tail}


def cut_down(z, n_docs):
    """The corpus restricted to its first n_docs documents (lists that lose every posting stay as empty lists)."""
    keep = z["post_doc"] < n_docs
    off = z["term_off"]
    cnt = [int(keep[off[t]:off[t + 1]].sum()) for t in range(len(off) - 1)]
    term_off = np.zeros(len(off), np.int64); term_off[1:] = np.cumsum(cnt)
    return dict(z, doc_ids=z["doc_ids"][:n_docs], doc_len=z["doc_len"][:n_docs], term_off=term_off,
                post_doc=z["post_doc"][keep], post_tf=z["post_tf"][keep])


def expected_rows(results, k):
    """[(doc, score)] of the oracle, one per distinct query -> padded (doc int32 [n, k], score float64 [n, k], n int32)."""
    doc = np.full((len(results), k), -1, np.int32)
    score = np.full((len(results), k), -np.inf, np.float64)
    n = np.zeros(len(results), np.int32)
    for i, (d, s) in enumerate(results):
        n[i] = len(d)
        doc[i, :len(d)] = d
        score[i, :len(d)] = s
    return doc, score, n
