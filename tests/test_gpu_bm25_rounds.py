"""BM25 scoring (bm25_taat_kernel) at the edges of its rank-indexed accumulators: touched counts of a span around the round cap,
the document that fills a round at a word, tile and span edge, slices of exactly R and R + 1 register-resident chunks, and
looked-up terms at every position of a query.  Calls of 16 rows run one tile per wave, calls of 1024 rows eight (the
benchmark's width); each case ASSERTS its split through DeviceEngine.bm25_split, then compares every row -- n, the documents,
the score bytes and the padding -- with oracle/bm25_ref.topk, and a query's row between the two widths.  Inputs:
tests/bm25_round_cases.py (checked on the CPU by test_bm25_round_cases.py).  No tolerance anywhere."""
import numpy as np
import pytest
import torch

import bm25_round_cases as rc
from msretr.docset import DocSet
from msretr.engine import DeviceEngine
from msretr.index import CorpusIndex
from oracle import bm25_ref
from within_ref import restrict_list

pytestmark = pytest.mark.gpu
N = rc.N_DOCS


class _Case:
    def __init__(self):
        assert torch.cuda.is_available(), "these tests need the MI355X"
        self.z, self.T = rc.build_corpus()
        self.queries, self.names = rc.build_queries(self.z, self.T)
        self.ix = CorpusIndex(total_docs=N, **self.z)
        self.eng = DeviceEngine(self.ix, max_queries=1024, max_k=1000)
        self._exp, self.rows = {}, {}

    def expected(self, k, ms):
        if (k, ms) not in self._exp:
            self._exp[(k, ms)] = rc.expected_rows([bm25_ref.topk(self.z, q, k, ms) for q in self.queries], k)
        return self._exp[(k, ms)]


@pytest.fixture(scope="module")
def case():
    c = _Case()
    yield c
    c.eng.close()


def _mismatch(case, what, idx, got, exp):
    doc, score, n = got
    e_doc, e_score, e_n = exp
    bad = (n != e_n) | (doc != e_doc).any(axis=1) | (score.view(np.int64) != e_score.view(np.int64)).any(axis=1)
    if bad.any():
        r = int(np.nonzero(bad)[0][0])
        col = np.nonzero((doc[r] != e_doc[r]) | (score[r].view(np.int64) != e_score[r].view(np.int64)))[0]
        c = int(col[0]) if len(col) else -1
        pytest.fail(f"{what}: {int(bad.sum())} of {len(n)} rows differ; first: row {r} = query '{case.names[idx[r]]}', n "
                    f"{int(n[r])} (expected {int(e_n[r])}), first differing rank {c}: document {int(doc[r, c])} score "
                    f"{score[r, c]!r}, expected document {int(e_doc[r, c])} score {e_score[r, c]!r}")


def _run(case, nq, k, ms):
    tpw, spans = rc.CALLS[nq]
    assert case.eng.bm25_split(nq) == (tpw, spans), f"{nq} rows no longer run {tpw} tiles per wave: re-derive the row counts"
    nd = len(case.queries)
    exp = case.expected(k, ms)
    rows = case.rows.setdefault((nq, k, ms), {})
    for start in rc.calls_for(nd, nq):
        idx = rc.fill(nd, nq, start)
        got = [x.cpu().numpy() for x in case.eng.bm25_topk([case.queries[i] for i in idx], k=k, min_score=ms)]
        _mismatch(case, f"nq={nq} k={k} min_score={ms} start={start}", idx, got, [e[idx] for e in exp])
        for r, i in enumerate(idx.tolist()):
            rows.setdefault(i, (got[0][r].tobytes(), got[1][r].tobytes(), int(got[2][r])))
    assert len(rows) == nd


@pytest.mark.parametrize("k,ms", rc.SETTINGS)
@pytest.mark.parametrize("nq", list(rc.CALLS))
def test_bm25_round_cases_vs_oracle(case, nq, k, ms):
    _run(case, nq, k, ms)


@pytest.mark.parametrize("k,ms", rc.SETTINGS)
def test_bm25_round_cases_do_not_depend_on_the_span_width(case, k, ms):
    for nq in rc.CALLS:
        if (nq, k, ms) not in case.rows:
            _run(case, nq, k, ms)
    one, eight = case.rows[(16, k, ms)], case.rows[(1024, k, ms)]
    for i, name in enumerate(case.names):
        assert one[i] == eight[i], (name, k, ms)


@pytest.mark.parametrize("nq", list(rc.CALLS))
def test_bm25_round_cases_within_a_document_set(case, nq):
    """The same queries restricted to every other document and to a block that crosses a tile and a span edge."""
    tpw, spans = rc.CALLS[nq]
    assert case.eng.bm25_split(nq) == (tpw, spans)
    k, ms = 300, 0.0
    other, block = np.zeros(N, bool), np.zeros(N, bool)
    other[::2] = True
    block[8000:8400] = True
    masks = [other, block]
    sets = [DocSet.from_mask(case.ix, m) for m in masks]
    nd = len(case.queries)
    full = [bm25_ref.topk(case.z, q, N, ms) for q in case.queries]
    for start in rc.calls_for(nd, nq):
        idx = rc.fill(nd, nq, start)
        which = [(r + r // nd) % 2 for r in range(nq)]
        exp = rc.expected_rows([restrict_list(full[i][0], full[i][1], len(full[i][0]), masks[w], k)
                                for i, w in zip(idx.tolist(), which)], k)
        got = [x.cpu().numpy() for x in case.eng.bm25_topk([case.queries[i] for i in idx], k=k, min_score=ms,
                                                            within=[sets[w] for w in which])]
        _mismatch(case, f"within nq={nq} start={start}", idx, got, exp)
