"""The segmented emit pass of the streaming dense scan (msr_gemm_f32_pass) against the one-launch pass
(MSR_CFG_SINGLE_EMIT) and the oracle.

One corpus for the whole module, built once and never changed: one chunk per document, 3 x 256 + 40 row tiles (807 tiles of
256 rows and a last tile of 100), k = 10.  On a 256-CU grid the rule cuts the pass at T1 = 256: a first segment of one grid
round, a rest of 552 tiles.  Planted in it (all unit rows):

* group A: 12 near-copies of one vector in 12 tiles of segment 1;
* group B: 12 near-copies of another in 12 tiles of segment 2, the last (short) tile among them;
* group T: 30 IDENTICAL rows, 15 in tiles of segment 1 and 15 in tiles of segment 2.

Engines are shared too (one per (max_queries, single_emit)); every test leaves them as it found them."""
import numpy as np
import pytest

from dense_geometry_cases import check_dense as _check_dense

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TILES, TAIL, K = 3 * 256 + 40, 100, 10
T1 = 256                                                        # tiles of segment 1 on a 256-CU grid


@pytest.fixture(scope="module")
def mods():
    from msretr.engine import DeviceEngine
    from msretr.index import CorpusIndex
    from oracle import dense_ref, rerank_ref
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return dict(DeviceEngine=DeviceEngine, CorpusIndex=CorpusIndex, dense_ref=dense_ref, rerank_ref=rerank_ref)


@pytest.fixture(scope="module")
def corpus(mods):
    C = (TILES - 1) * 256 + TAIL
    emb_t = torch.randn((C, 768), generator=torch.Generator().manual_seed(808))
    emb = emb_t.numpy()
    rng = np.random.default_rng(808)
    va, vb, vt = [v / np.linalg.norm(v) for v in rng.standard_normal((3, 768)).astype(np.float32)]
    tiles_a = np.arange(3, 3 + 12 * 20, 20)                                          # 3 .. 223: segment 1
    tiles_b = np.concatenate([np.arange(300, 300 + 11 * 45, 45), [TILES - 1]])       # 300 .. 750 and the last tile
    rows_a, rows_b = tiles_a * 256 + 17, tiles_b * 256 + 5
    emb[rows_a] = va + 0.5 * emb[rows_a] / np.linalg.norm(emb[rows_a], axis=1, keepdims=True)
    emb[rows_b] = vb + 0.5 * emb[rows_b] / np.linalg.norm(emb[rows_b], axis=1, keepdims=True)
    tiles_t = np.concatenate([np.arange(10, 10 + 15 * 16, 16), np.arange(260, 260 + 15 * 36, 36)])   # 10 .. 234 | 260 .. 764
    rows_t = tiles_t * 256 + 201
    emb[rows_t] = vt
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)
    assert tiles_a.max() < T1 <= tiles_b.min() and (tiles_t < T1).sum() == 15
    doc_off = np.arange(C + 1, dtype=np.int64)
    ix = mods["CorpusIndex"](doc_ids=np.arange(C, dtype=np.int64), doc_off=doc_off.astype(np.int32),
                             chunk_ids=np.arange(C, dtype=np.int64), emb=emb, total_docs=C)
    q = rng.standard_normal((300, 768)).astype(np.float32) * rng.uniform(0.5, 8, size=(300, 1)).astype(np.float32)
    q[2:30] = emb[rng.integers(0, C, 28)] + 0.4 * q[2:30] / np.linalg.norm(q[2:30], axis=1, keepdims=True)
    q[0] = va * 2.0                                             # every top-k document inside segment 1
    q[1] = vb * 0.7                                             # ... inside segment 2
    q[64] = vt * 1.5                                            # the tie group: 30 documents at exactly the same score
    q[65] = emb[C - 1] * 0.8                                    # the last row of the last, short tile
    q.setflags(write=False)
    return dict(ix=ix, emb=emb, doc_off=doc_off, C=C, q=q, rows_a=rows_a, rows_b=rows_b, rows_t=rows_t)


@pytest.fixture(scope="module")
def engines(mods, corpus):
    made = {}

    def get(max_q, single):
        if (max_q, single) not in made:
            made[(max_q, single)] = mods["DeviceEngine"](corpus["ix"], max_queries=max_q, max_k=100, rerank_max_docs=0,
                                                         single_emit=single)
        return made[(max_q, single)]
    yield get
    for e in made.values():
        e.close()


def _segmented_or_skip(eng):
    seg, entries = eng.dense_pass_info()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if seg == 1 and cus != 256:
        pytest.skip(f"{cus} compute units: the rule leaves this corpus in one segment (the shape is laid out for a 256-CU grid)")
    assert seg >= 2, (seg, cus)
    return entries


def _np(got):
    return [x.cpu().numpy() for x in got]


PICK = [0, 1, 2, 40, 64, 65]


@pytest.mark.parametrize("max_q,Q,width", [(256, 129, 256), (256, 256, 256), (128, 100, 128), (512, 300, 256)])
def test_segmented_pass_equals_single_emit_and_the_oracle(mods, corpus, engines, max_q, Q, width):
    """Main shape, both kernel widths, one and two query groups per launch (300 queries on a 512-query engine: the f16
    image): at least two emit launches, every output array bit-equal to the single-emit engine's, the oracle's answer for a
    handful of queries (the adversarial ones among them), and strictly fewer entries in the wave buffers."""
    q = corpus["q"][:Q]
    seg_eng, one_eng = engines(max_q, False), engines(max_q, True)
    got = seg_eng.dense_topk(q, k=K)
    assert seg_eng.dense_path() == width
    n_seg = _segmented_or_skip(seg_eng)
    ref = one_eng.dense_topk(q, k=K)
    assert one_eng.dense_path() == width
    seg1, n_one = one_eng.dense_pass_info()
    assert seg1 == 1
    g, r = _np(got), _np(ref)
    assert all(np.array_equal(a, b) for a, b in zip(g, r))
    pick = [i for i in PICK if i < Q]
    _check_dense(mods, seg_eng, corpus["doc_off"], corpus["emb"], q[pick], K, 0, [x[pick] for x in got])
    print(f"entries max_queries={max_q} Q={Q}: segmented {n_seg} single {n_one} ratio {n_seg / max(n_one, 1):.3f}")
    assert 0 < n_seg < n_one
    assert bool((g[3] == K).all())                              # (nobody went back to the sweeps)


def test_adversarial_placements_of_the_winners(mods, corpus, engines):
    """Queries that are scaled copies of planted rows, in one 100-query call of the 128-query kernel and one 256-query call:
    all top-k documents in segment 1 (the refreshed threshold is as high as it gets), all in segment 2 (the refresh barely
    moves), 30 identical rows over both segments with k = 10 (the threshold sits at the tie value: >= and the f16 round-down
    keep them; ties order by ascending document), and the last row of the short last tile."""
    emb, C = corpus["emb"], corpus["C"]
    for max_q, Q in ((128, 100), (256, 256)):
        eng = engines(max_q, False)
        got = eng.dense_topk(corpus["q"][:Q], k=K)
        _segmented_or_skip(eng)
        doc, score, chunk, n = _np(got)
        assert set(doc[0].tolist()) <= set(corpus["rows_a"].tolist()) and doc[0].max() < T1 * 256
        assert set(doc[1].tolist()) <= set(corpus["rows_b"].tolist()) and doc[1].min() >= T1 * 256
        assert doc[64].tolist() == np.sort(corpus["rows_t"])[:K].tolist()             # the ten lowest documents of the tie
        assert np.all(score[64] == score[64, 0]) and abs(score[64, 0] - 1.0) <= 1e-5
        assert doc[65, 0] == C - 1 and chunk[65, 0] == C - 1 and abs(score[65, 0] - 1.0) <= 1e-5
        assert np.array_equal(doc, chunk)                       # one chunk per document
        _check_dense(mods, eng, corpus["doc_off"], emb, corpus["q"][[0, 1, 64, 65]], K, 0, [x[[0, 1, 64, 65]] for x in got])
        assert all(np.array_equal(a, b) for a, b in zip(_np(got), _np(engines(max_q, True).dense_topk(corpus["q"][:Q], k=K))))


def test_overflow_goes_to_the_gated_sweeps_as_before(mods, corpus, engines):
    """A zero query (every cosine 0: a tie group of the whole corpus) in a 100-query batch overflows its candidate list on
    both engines alike: only its own 64-query slice comes back from the gated sweeps, the other slice is the pass' answer,
    bit-equal to the single-emit engine's."""
    qz = corpus["q"][:100].copy()
    qz[1] = 0.0
    eng, one = engines(128, False), engines(128, True)
    got = eng.dense_topk(qz, k=K)
    _segmented_or_skip(eng)
    gz, rz = _np(got), _np(one.dense_topk(qz, k=K))
    assert all(np.array_equal(a, b) for a, b in zip(gz, rz))
    sw = _np(eng.dense_topk(qz[:64], k=K))                     # a 64-query call runs on the sweeps
    assert eng.dense_path() == 64 and eng.dense_pass_info() == (0, 0)
    ps = _np(eng.dense_topk(corpus["q"][:100], k=K))            # the batch without the zero query: nothing overflows
    assert all(np.array_equal(a[:64], b) for a, b in zip(gz, sw))
    assert all(np.array_equal(a[64:], b[64:]) for a, b in zip(gz, ps))
    assert not np.array_equal(gz[1][:64], ps[1][:64])           # (sweep scores differ from the pass' exact cosines in the last bits)
    _check_dense(mods, eng, corpus["doc_off"], corpus["emb"], qz[[0, 1, 70]], K, 0, [x[[0, 1, 70]] for x in got])


def test_sharded_entry_points_equal_single_emit(corpus, engines):
    """dense_begin(k_part) + dense_end(bound) on the main shape: the value dense_begin returns and every output array equal
    the single-emit engine's bit for bit, with and without a bound."""
    q = corpus["q"][:256]
    eng, one = engines(256, False), engines(256, True)
    for k_part in (K, 3):
        part = eng.dense_begin(q, k=K, k_part=k_part)
        _segmented_or_skip(eng)
        part_ref = one.dense_begin(q, k=K, k_part=k_part)
        assert one.dense_pass_info()[0] == 1
        assert np.array_equal(part.cpu().numpy(), part_ref.cpu().numpy())
        bound = None if k_part == K else part + 0.01            # (a bound above this shard's own: fewer than k documents come back)
        got, ref = _np(eng.dense_end(256, k=K, bound=bound)), _np(one.dense_end(256, k=K, bound=bound))
        assert all(np.array_equal(a, b) for a, b in zip(got, ref))
        assert bool((got[3] == K).all()) if bound is None else bool((got[3] <= K).all() and (got[3] < K).any())
