"""BM25 scoring (bm25_taat_kernel) and its list select at every span width.  A wave of the scoring kernel walks tpw = 1, 2, 4
or 8 consecutive 1024-document tiles; the number of queries in the call picks tpw, and the select behind it then gives a
workgroup one, several or no segment of a query's candidate row.  Every case first ASSERTS the split it is named after through
DeviceEngine.bm25_split (msr_debug_bm25_split), then compares every row of the call -- n, the documents, the scores and the
padding -- bit for bit with oracle/bm25_ref.topk.  Inputs: tests/bm25_span_cases.py (checked on the CPU by
test_bm25_span_cases.py).  No tolerance anywhere."""
import numpy as np
import pytest
import torch

import bm25_span_cases as sc
from msretr.docset import DocSet
from msretr.engine import DeviceEngine
from msretr.index import CorpusIndex
from oracle import bm25_ref
from within_ref import restrict_list

pytestmark = pytest.mark.gpu
N, TILE = sc.N_DOCS, sc.TILE
WIDTHS = list(sc.WIDTH_CASES)
ONE_PER_WIDTH = {1: 16, 2: 265, 4: 512, 8: 1024}              # the calls the width-invariance check compares


class _Case:
    def __init__(self):
        assert torch.cuda.is_available(), "these tests need the MI355X"
        self.z, self.T = sc.build_corpus()
        self.queries, self.names = sc.build_queries(self.z, self.T)
        self.ix = CorpusIndex(total_docs=N, **self.z)
        self.eng = DeviceEngine(self.ix, max_queries=1024, max_k=1000)
        self._exp, self._full, self.first_rows = {}, {}, {}

    def expected(self, k, ms):
        """The oracle's rows of the distinct queries, padded: evaluated once per setting."""
        if (k, ms) not in self._exp:
            self._exp[(k, ms)] = sc.expected_rows([bm25_ref.topk(self.z, q, k, ms) for q in self.queries], k)
        return self._exp[(k, ms)]

    def full(self, ms):
        """Every accepted document of every distinct query, in the unrestricted order (the oracle with k = N)."""
        if ms not in self._full:
            self._full[ms] = [bm25_ref.topk(self.z, q, N, ms) for q in self.queries]
        return self._full[ms]


@pytest.fixture(scope="module")
def case():
    c = _Case()
    yield c
    c.eng.close()


def _assert_split(eng, nq):
    tpw, spans, last, parts, per = sc.WIDTH_CASES[nq]
    assert eng.bm25_split(nq) == (tpw, spans), f"{nq} queries no longer run {tpw} tiles per wave: re-derive the query counts"
    assert 61 - (spans - 1) * tpw == last
    return tpw


def _compare(case, got, idx, exp, what):
    """Every row of the call against the expected row of its distinct query, bytes and padding included."""
    doc, score, n = [x.cpu().numpy() for x in got]
    e_doc, e_score, e_n = exp[0][idx], exp[1][idx], exp[2][idx]
    bad = (n != e_n) | (doc != e_doc).any(axis=1) | (score.view(np.int64) != e_score.view(np.int64)).any(axis=1)
    if bad.any():
        r = int(np.nonzero(bad)[0][0])
        col = np.nonzero((doc[r] != e_doc[r]) | (score[r].view(np.int64) != e_score[r].view(np.int64)))[0]
        c = int(col[0]) if len(col) else -1
        d_got, d_exp = (int(doc[r, c]), int(e_doc[r, c])) if c >= 0 else (None, None)
        pytest.fail(f"{what}: {int(bad.sum())} of {len(n)} rows differ; first: row {r} = query '{case.names[idx[r]]}' "
                    f"{case.queries[idx[r]][:8]}..., n {int(n[r])} (expected {int(e_n[r])}), first differing rank {c}: document "
                    f"{d_got} (tile {None if d_got is None else d_got // TILE}) score {score[r, c] if c >= 0 else None!r}, expected "
                    f"document {d_exp} (tile {None if d_exp is None else d_exp // TILE}) score "
                    f"{e_score[r, c] if c >= 0 else None!r}")
    # (equal arrays: n, documents, score bytes and the -1 / -inf padding behind n all match)
    return doc, score, n


def _run(case, nq, k, ms):
    """The calls of nq rows that together run every distinct query (one call when nq >= their number), all rows compared."""
    nd = len(case.queries)
    exp = case.expected(k, ms)
    for start in sc.calls_for(nd, nq):
        idx = sc.fill(nd, nq, start)
        got = case.eng.bm25_topk([case.queries[i] for i in idx], k=k, min_score=ms)
        doc, score, n = _compare(case, got, idx, exp, f"nq={nq} k={k} min_score={ms} start={start}")
        rows = case.first_rows.setdefault((nq, k, ms), {})
        for r, i in enumerate(idx.tolist()):
            if i not in rows:
                rows[i] = (doc[r].tobytes(), score[r].tobytes(), int(n[r]))


@pytest.mark.parametrize("k,ms", sc.SETTINGS)
@pytest.mark.parametrize("nq", WIDTHS)
def test_bm25_rows_at_every_span_width_vs_oracle(case, nq, k, ms):
    _assert_split(case.eng, nq)
    _run(case, nq, k, ms)


@pytest.mark.parametrize("k,ms", sc.SETTINGS)
def test_bm25_rows_do_not_depend_on_the_span_width(case, k, ms):
    """The row of a distinct query is byte-identical at tpw = 1, 2, 4 and 8: the result does not depend on the work split."""
    rows = {}
    for tpw, nq in ONE_PER_WIDTH.items():
        assert case.eng.bm25_split(nq)[0] == tpw
        if (nq, k, ms) not in case.first_rows:
            _run(case, nq, k, ms)
        rows[tpw] = case.first_rows[(nq, k, ms)]
    for i, name in enumerate(case.names):
        for tpw in (2, 4, 8):
            assert rows[tpw][i] == rows[1][i], (name, tpw, k, ms)


@pytest.mark.parametrize("ms", [0.0, -1e9])
@pytest.mark.parametrize("nq", WIDTHS)
def test_bm25_within_document_sets_at_every_span_width(case, nq, ms):
    """The same queries restricted to document sets, a per-query mix: None, the empty set, one document, every other document,
    a block that crosses a tile and a span edge, the last partial 32-bit word.  Expected: the oracle's full list of the query,
    restricted by the mask and cut (within_ref.restrict_list)."""
    _assert_split(case.eng, nq)
    k = 300
    masks = sc.within_masks()
    names = list(masks)
    sets = {s: (None if masks[s] is None else DocSet.from_mask(case.ix, masks[s])) for s in names}
    nd = len(case.queries)
    full = case.full(ms)
    exp = {}
    for start in sc.calls_for(nd, nq):
        idx = sc.fill(nd, nq, start)
        # neighbouring rows run different sets, and a query meets the next set at each of its positions in the call
        which = [names[(r % nd + r // nd) % len(names)] for r in range(nq)]
        pairs = sorted(set(zip(idx.tolist(), which)))
        for p in pairs:
            if p not in exp:
                fd, fs = full[p[0]]
                exp[p] = (fd[:k], fs[:k]) if masks[p[1]] is None else restrict_list(fd, fs, len(fd), masks[p[1]], k)
        e = sc.expected_rows([exp[p] for p in pairs], k)
        row_of = {p: j for j, p in enumerate(pairs)}
        sel = np.array([row_of[(i, s)] for i, s in zip(idx.tolist(), which)])
        got = case.eng.bm25_topk([case.queries[i] for i in idx], k=k, min_score=ms, within=[sets[s] for s in which])
        doc, score, n = [x.cpu().numpy() for x in got]
        e_doc, e_score, e_n = e[0][sel], e[1][sel], e[2][sel]
        bad = (n != e_n) | (doc != e_doc).any(axis=1) | (score.view(np.int64) != e_score.view(np.int64)).any(axis=1)
        if bad.any():
            r = int(np.nonzero(bad)[0][0])
            pytest.fail(f"nq={nq} min_score={ms} start={start}: {int(bad.sum())} of {nq} rows differ; first: row {r} = query "
                        f"'{case.names[idx[r]]}' within '{which[r]}': n {int(n[r])} (expected {int(e_n[r])}), documents "
                        f"{doc[r, :6].tolist()} (expected {e_doc[r, :6].tolist()})")
        if nq >= len(names) * nd:                                # every (query, set) pair has run
            assert len(exp) == nd * len(names)
    for s in ("empty",):
        assert all(len(v[0]) == 0 for p, v in exp.items() if p[1] == s)


def _tie_engine(tf):
    ix = CorpusIndex(doc_ids=np.arange(N, dtype=np.int64), doc_len=np.full(N, 7, np.int32), term_off=np.array([0, N], np.int64),
                     post_doc=np.arange(N, dtype=np.int32), post_tf=tf, idf=np.array([0.8], np.float32), avgdl=7.0,
                     total_docs=N)
    z = dict(doc_ids=np.arange(N, dtype=np.int64), doc_len=np.full(N, 7, np.int32), term_off=np.array([0, N], np.int64),
             post_doc=np.arange(N, dtype=np.int32), post_tf=tf, idf=np.array([0.8], np.float32), avgdl=7.0)
    return DeviceEngine(ix, max_queries=1024, max_k=1000), z


def test_bm25_ties_at_width_8():
    """One term in every document, equal tf and length: 61 957 equal scores per row, far more than the select's exact sort
    holds (MSR_SEL_CAP), so sel_final_kernel finishes in-kernel over rows of 8 segments, 4 per workgroup.  Then two score
    levels with the cut inside the second tie group."""
    assert torch.cuda.is_available(), "these tests need the MI355X"
    eng, z = _tie_engine(np.full(N, 2, np.int32))
    assert eng.bm25_split(1024) == (8, 8) and sc.select_parts(8, 1024) == (2, 4)
    doc, score, n = [x.cpu().numpy() for x in eng.bm25_topk([[0]] * 1024, k=1000)]
    od, os_ = bm25_ref.topk(z, [0], 1000)
    assert od.tolist() == list(range(1000)) and len(set(os_.tolist())) == 1
    assert (n == 1000).all() and (doc == np.arange(1000, dtype=np.int32)[None, :]).all()
    assert (score.view(np.int64) == os_.view(np.int64)[None, :]).all()
    eng.close()
    # two levels: 600 documents spread over every span score higher; the other 400 come from the 61 357 that tie below them
    tf = np.full(N, 1, np.int32)
    high = np.sort(np.random.default_rng(5).choice(N, size=600, replace=False))
    tf[high] = 3
    eng, z = _tie_engine(tf)
    assert eng.bm25_split(1024) == (8, 8)
    doc, score, n = [x.cpu().numpy() for x in eng.bm25_topk([[0]] * 1024, k=1000)]
    od, os_ = bm25_ref.topk(z, [0], 1000)
    low = np.setdiff1d(np.arange(N), high)[:400]
    assert od.tolist() == high.tolist() + low.tolist() and len(set(os_.tolist())) == 2
    assert (n == 1000).all() and (doc == od.astype(np.int32)[None, :]).all()
    assert (score.view(np.int64) == os_.view(np.int64)[None, :]).all()
    eng.close()


def test_bm25_split_export_refusals(case):
    eng = case.eng
    assert eng.bm25_split(1) == (1, 61)
    from msretr._abi import MsrError
    for bad in (0, -1, 1025):
        with pytest.raises(MsrError):
            eng.bm25_split(bad)
