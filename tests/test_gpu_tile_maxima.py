"""The join of the streaming dense pass' tile maxima (gemm_tmax_kernel of msr_gemm.hip: maximum over the parts of a tile,
transposed into one row per query) at its edges, through msr_dense_topk: 129 and 256 queries are one group of the 256-query
f32 kernel (8 parts per tile, one per wave), 300 queries two groups in one launch over the 16-bit row image (one part).  One
chunk per document, so a corpus of T x 256 (+ a tail of) rows is T (+ 1) row tiles: 64 tiles are two full blocks of the
32-tile transpose, 65 leave one tile for a third block, 95 a ragged one; the sample pass joins every 2nd or 3rd tile (32
of them).  k = 10, so that there are at least 2 k tiles and the streaming path is taken (asserted with dense_path()).

A wrong or missing tile maximum moves the k-th-maximum thresholds: too high and true neighbours are never emitted, garbage
and the pass overflows or drops them.  So the check is the result: it must equal a torch f32 computation of the same
cosines under the rule of the dense parity tests (tests/test_gpu_parity.py, _check_dense): scores within 1e-5, descending,
the same documents except for swaps among scores within 2e-5 of the k-th, exact ties by ascending document."""
import numpy as np
import pytest
import torch

from msretr.engine import DeviceEngine
from msretr.index import CorpusIndex

pytestmark = pytest.mark.gpu

K = 10
CORPORA = {64: 64 * 256, 65: 64 * 256 + 9, 95: 94 * 256 + 100}       # tiles -> rows (= documents)


@pytest.fixture(scope="module")
def queries():
    q = torch.randn((300, 768), generator=torch.Generator().manual_seed(23)) * 3.0
    return q.numpy()


@pytest.fixture(scope="module", params=sorted(CORPORA))
def corpus(request, queries):
    """(tiles, index, unit rows on the device); some queries are (near) copies of rows in the first, an inner and the last tile"""
    assert torch.cuda.is_available(), "these tests need the MI355X"
    tiles, rows = request.param, CORPORA[request.param]
    emb = torch.randn((rows, 768), generator=torch.Generator().manual_seed(tiles))
    emb /= emb.norm(dim=1, keepdim=True)
    emb = emb.numpy()
    ix = CorpusIndex(doc_ids=np.arange(rows, dtype=np.int64), doc_off=np.arange(rows + 1, dtype=np.int32),
                     chunk_ids=np.arange(rows, dtype=np.int64), emb=emb, total_docs=rows)
    return tiles, ix, torch.from_numpy(emb).cuda()


def _queries_for(queries, emb_dev, nq):
    q = queries[:nq].copy()
    rows = emb_dev.shape[0]
    e = lambda r: emb_dev[r].cpu().numpy()
    q[0] = e(0) * 2.0                                             # first row of the first tile
    q[1] = e(rows - 1) * 0.5                                      # last row of the last (short) tile
    q[nq - 1] = e(33 * 256 + 7) + 0.02 * q[nq - 1]                # near a row of an inner tile, from the last query of the call
    q[2] = e(63 * 256 + 255) * 7.0                                # last row of the last tile of the second transpose block
    return q


def _check(q, emb_dev, got):
    doc, score, chunk, n = [x.cpu().numpy() for x in got]
    qd = torch.from_numpy(q).cuda()
    cos = (qd / qd.norm(dim=1, keepdim=True)) @ emb_dev.T         # f32; one chunk per document: the document's score
    ref_s, ref_d = torch.topk(cos, K, dim=1)
    cos, ref_s, ref_d = cos.cpu().numpy(), ref_s.cpu().numpy(), ref_d.cpu().numpy()
    for i in range(q.shape[0]):
        assert n[i] == K, (i, int(n[i]))
        np.testing.assert_allclose(score[i], ref_s[i], rtol=0, atol=1e-5)
        np.testing.assert_allclose(score[i], cos[i, doc[i]], rtol=0, atol=1e-5)
        assert np.all(np.diff(score[i]) <= 0)
        for d in set(doc[i].tolist()) ^ set(ref_d[i].tolist()):   # swaps among scores closer than the tolerance only
            assert abs(cos[i, d] - ref_s[i, -1]) <= 2e-5, (i, d)
        for j in range(1, K):
            if score[i, j] == score[i, j - 1]:
                assert doc[i, j] > doc[i, j - 1]
        assert chunk[i].tolist() == doc[i].tolist()


@pytest.mark.parametrize("nq,max_queries", [(129, 256), (256, 256), (300, 512)])
def test_dense_topk_through_the_tile_maxima_join(corpus, queries, nq, max_queries):
    tiles, ix, emb_dev = corpus
    eng = DeviceEngine(ix, max_queries=max_queries, max_k=K, rerank_max_docs=0)
    assert eng.scan_width() == 256
    q = _queries_for(queries, emb_dev, nq)
    got = eng.dense_topk(q, k=K)
    assert eng.dense_path() == 256, (tiles, nq, eng.dense_path())
    if nq == 300:
        assert eng.row_image_state() == "built"                    # two groups in one launch: one part per tile
    _check(q, emb_dev, got)
    doc = got[0].cpu().numpy()
    assert doc[0, 0] == 0 and doc[1, 0] == emb_dev.shape[0] - 1 and doc[nq - 1, 0] == 33 * 256 + 7 and doc[2, 0] == 63 * 256 + 255
    eng.close()
