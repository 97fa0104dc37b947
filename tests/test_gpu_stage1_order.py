"""The ITEM ORDER of the BM25 scoring kernel.  A plan kernel in front of bm25_taat_kernel weighs every query of a slice by the
postings the scoring kernel will stream for it and orders the slice: the items of the HEAVY queries (expected postings per
item above the BM25_RES resident chunks: weight * span documents > BM25_RES * 64 * n_docs) first, then the others; the
segment an item writes is still the one of its true (query, span).  A query's row must depend on neither: every row of every
call below is compared bit for bit with oracle/bm25_ref.topk, and the same batch presented in REVERSED order must give
byte-identical rows.

The slices are built from a numpy restatement of the weight (heavy_set below; R and the tile size are read from the sources)
on the 61-tile corpus of bm25_span_cases.py, at 1024 queries (8 tiles per item) and at 16 (1 tile per item), the split
asserted first through DeviceEngine.bm25_split: every query heavy / none / exactly one, placed first and placed last / all
weights equal (distinct queries, then one query repeated) / queries without a streamed term, with unknown terms only and
empty ones among the light / a call of more queries than max_queries, whose later slices start at q_first != 0 with another
heavy set and another width / min_score 0 and -0.5 (which streams every list: other weights) / document sets per query."""
import numpy as np
import pytest
import torch

import bm25_round_cases as rc
import bm25_span_cases as sc
from msretr.docset import DocSet
from msretr.engine import DeviceEngine
from msretr.index import CorpusIndex
from oracle import bm25_ref
from within_ref import restrict_list

pytestmark = pytest.mark.gpu
N, TILE, K = sc.N_DOCS, sc.TILE, 200
RES = rc.resident_chunks()
SPLITS = {1024: (8, 8), 16: (1, 61), 8: (1, 61)}                # queries of a slice -> (tiles per item, spans)
MIN_SCORES = (0.0, -0.5)


class _Case:
    def __init__(self):
        assert torch.cuda.is_available(), "these tests need the MI355X"
        self.z, self.T = sc.build_corpus()
        queries, names = sc.build_queries(self.z, self.T)
        V = len(self.z["idf"])
        for i, t in enumerate(self.T["short"]):                  # nine distinct queries of one 30-posting list each
            queries.append([t]); names.append("short_%d" % i)
        queries.append([V + 110, -3]); names.append("unknown_only")
        self.queries, self.names = queries, names
        self.ix = CorpusIndex(total_docs=N, **self.z)
        self.eng = DeviceEngine(self.ix, max_queries=1024, max_k=K)
        self.eng16 = DeviceEngine(self.ix, max_queries=16, max_k=K)
        self._full = {}
        off = self.z["term_off"]
        self.df = off[1:] - off[:-1]
        self.tabled = set(self.T["neg_tabled"])

    def full(self, ms):
        """Every accepted document of every distinct query in order (the oracle with k = N), evaluated once per min_score."""
        if ms not in self._full:
            self._full[ms] = [bm25_ref.topk(self.z, q, N, ms) for q in self.queries]
        return self._full[ms]

    def weight(self, i, ms):
        """Postings of the lists the scoring kernel streams for distinct query i: every known, non-empty list except the
        negative ones with a dense table when min_score >= 0."""
        w = 0
        for t in dict.fromkeys(self.queries[i]):
            if 0 <= t < len(self.df) and self.df[t] > 0 and not (ms >= 0 and t in self.tabled and self.z["idf"][t] < 0):
                w += int(self.df[t])
        return w

    def heavy_set(self, ms, tpw):
        w = np.array([self.weight(i, ms) for i in range(len(self.queries))])
        return w, w * tpw * TILE > RES * 64 * N

    def close(self):
        self.eng.close()
        self.eng16.close()


@pytest.fixture(scope="module")
def case():
    c = _Case()
    yield c
    c.close()


def _cycle(members, n):
    return [members[j % len(members)] for j in range(n)]


def _slices(case, nq, ms):
    """name -> the distinct query of every row of a slice of nq rows."""
    tpw = SPLITS[nq][0]
    w, heavy = case.heavy_set(ms, tpw)
    H, L = np.nonzero(heavy)[0].tolist(), np.nonzero(~heavy)[0].tolist()
    name = {n: i for i, n in enumerate(case.names)}
    assert len(H) >= 4 and len(L) >= 8
    # among the light: no streamed term at min_score >= 0 (weight 0), unknown terms only, no term at all
    for n in ("neg_alone", "unknown_only", "empty") if ms >= 0 else ("unknown_only", "empty"):
        assert name[n] in L and w[name[n]] == 0, n
    singles = [name["short_%d" % i] for i in range(9)]
    assert len({int(w[i]) for i in singles}) == 1 and not heavy[singles].any()
    out = {
        "every_query_heavy": _cycle(H, nq),
        "none_heavy": _cycle(L, nq),
        "one_heavy_first": [H[0]] + _cycle(L, nq - 1),
        "one_heavy_last": _cycle(L, nq - 1) + [H[-1]],
        "equal_weights": _cycle(singles, nq),
        "one_query_repeated": [H[1]] * nq,
        "mixed": sc.fill(len(case.queries), nq).tolist(),
    }
    assert heavy[out["every_query_heavy"]].all() and not heavy[out["none_heavy"]].any()
    assert heavy[out["one_heavy_first"]].sum() == 1 == heavy[out["one_heavy_last"]].sum()
    assert 0 < heavy[out["mixed"]].sum() < nq
    return out


def _expected(case, idx, ms, masks=None):
    full = case.full(ms)
    rows = []
    for r, i in enumerate(idx):
        fd, fs = full[i]
        m = None if masks is None else masks[r]
        rows.append((fd[:K], fs[:K]) if m is None else restrict_list(fd, fs, len(fd), m, K))
    return sc.expected_rows(rows, K)


def _call(eng, case, idx, ms, sets=None):
    got = eng.bm25_topk([case.queries[i] for i in idx], k=K, min_score=ms, within=sets)
    return [x.cpu().numpy() for x in got]


def _check(case, eng, idx, ms, what, sets=None, masks=None):
    """The call against the oracle, then the reversed call against the call: bytes and padding included."""
    doc, score, n = _call(eng, case, idx, ms, sets)
    e_doc, e_score, e_n = _expected(case, idx, ms, masks)
    bad = (n != e_n) | (doc != e_doc).any(axis=1) | (score.view(np.int64) != e_score.view(np.int64)).any(axis=1)
    if bad.any():
        r = int(np.nonzero(bad)[0][0])
        pytest.fail(f"{what}: {int(bad.sum())} of {len(n)} rows differ from the oracle; first: row {r} = query "
                    f"'{case.names[idx[r]]}', n {int(n[r])} (expected {int(e_n[r])}), documents {doc[r, :6].tolist()} "
                    f"(expected {e_doc[r, :6].tolist()})")
    rdoc, rscore, rn = _call(eng, case, idx[::-1], ms, None if sets is None else sets[::-1])
    assert rdoc[::-1].tobytes() == doc.tobytes() and rscore[::-1].tobytes() == score.tobytes() and \
        rn[::-1].tobytes() == n.tobytes(), f"{what}: the reversed batch gives other rows"


@pytest.mark.parametrize("ms", MIN_SCORES)
@pytest.mark.parametrize("nq", [1024, 16])
def test_rows_do_not_depend_on_the_item_order(case, nq, ms):
    assert case.eng.bm25_split(nq) == SPLITS[nq], f"{nq} queries no longer run {SPLITS[nq][0]} tiles per item"
    for name, idx in _slices(case, nq, ms).items():
        _check(case, case.eng, idx, ms, f"nq={nq} min_score={ms} {name}")


@pytest.mark.parametrize("ms", MIN_SCORES)
def test_later_slices_of_a_call_have_their_own_order(case, ms):
    """n_queries > max_queries: 1024 + 16 rows on the 1024-query engine (a slice of 8 tiles per item without a heavy query,
    then one of 1 tile per item at q_first = 1024 with its own heavy set); 16 + 16 + 8 rows on a 16-query engine (every query
    heavy / none / one heavy, placed last)."""
    assert case.eng.bm25_split(1024) == SPLITS[1024] and case.eng.bm25_split(16) == SPLITS[16]
    big, small = _slices(case, 1024, ms), _slices(case, 16, ms)
    _check(case, case.eng, big["none_heavy"] + small["mixed"], ms, f"1024+16 min_score={ms}")
    assert case.eng16.bm25_split(16) == SPLITS[16] and case.eng16.bm25_split(8) == SPLITS[8]
    idx = small["every_query_heavy"] + small["none_heavy"] + _slices(case, 8, ms)["one_heavy_last"]
    _check(case, case.eng16, idx, ms, f"16+16+8 min_score={ms}")


@pytest.mark.parametrize("nq", [1024, 16])
def test_document_sets_with_the_item_order(case, nq):
    """The restricted instantiation of the scoring kernel: a per-row mix of no set, the empty set, one document, every other
    document, a block across a span edge, the last partial word.  Expected: the oracle's full list, restricted and cut."""
    assert case.eng.bm25_split(nq) == SPLITS[nq]
    masks = sc.within_masks()
    names = list(masks)
    sets = {s: (None if masks[s] is None else DocSet.from_mask(case.ix, masks[s])) for s in names}
    for name in ("mixed", "one_heavy_last"):
        idx = _slices(case, nq, 0.0)[name]
        which = [names[(r + r // len(names)) % len(names)] for r in range(nq)]
        _check(case, case.eng, idx, 0.0, f"within nq={nq} {name}", sets=[sets[s] for s in which],
               masks=[masks[s] for s in which])
