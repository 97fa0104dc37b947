"""Tile maxima taken from the emitted entries (msr_gemm_f32_pass): the 256-query emit pass over the f32
rows stores none, the selects behind it read what gemm_entry_tmax_kernel joins out of the wave buffers.

The corpus shape of tests/test_gpu_dense_segments.py, built here and never changed: one chunk per document, 3 x 256 + 40 row
tiles (807 of 256 rows and a last one of 100), k = 10, so that a 256-CU grid cuts the pass at T1 = 256.  Every row carries a
common component 6 u (u a unit vector): the cosine of EVERY row with -u is negative, which gives the module a query whose
thresholds and tile maxima are all negative -- the unsigned-minimum branch of the atomic join decides its result.  Planted:

* group A: 12 near-copies of one vector in 12 tiles of segment 1;
* group B: 12 near-copies of another in 12 tiles of segment 2, the last (short) tile among them.

Which product configurations launch the f32-row emit instantiations with SEVERAL query groups: an engine for >= 512 queries
per call that holds no f16 image of the rows -- row_copy=False (MSR_CFG_NO_ROW_COPY), or an image whose allocation failed at
bind time.  The first is covered below (300 queries on a 512-query engine: two groups in one launch, entries of both joined
in one walk); every other multi-group launch reads the f16 image and joins its maxima in LDS as before.

Engines are shared (one per (max_queries, single_emit, row_copy)); every test leaves them as it found them."""
import numpy as np
import pytest

from dense_geometry_cases import check_dense as _check_dense

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TILES, TAIL, K = 3 * 256 + 40, 100, 10
T1 = 256                                                        # tiles of segment 1 on a 256-CU grid
Q_A, Q_B, Q_NEG, Q_LAST = 0, 1, 3, 5                            # the planted queries' places in the batch


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
    rng = np.random.default_rng(811)
    u = rng.standard_normal(768).astype(np.float32)
    u /= np.linalg.norm(u)
    emb = torch.randn((C, 768), generator=torch.Generator().manual_seed(811)).numpy()
    emb += np.float32(6.0) * u
    va, vb = [v / np.linalg.norm(v) for v in (rng.standard_normal((2, 768)).astype(np.float32) + np.float32(6.0) * u)]
    tiles_a = np.arange(3, 3 + 12 * 20, 20)                                          # 3 .. 223: segment 1
    tiles_b = np.concatenate([np.arange(300, 300 + 11 * 45, 45), [TILES - 1]])       # 300 .. 750 and the last tile
    rows_a, rows_b = tiles_a * 256 + 17, tiles_b * 256 + 5
    unit = lambda x: x / np.linalg.norm(x, axis=1, keepdims=True)
    emb[rows_a] = va + 0.5 * unit(rng.standard_normal((12, 768)).astype(np.float32))
    emb[rows_b] = vb + 0.5 * unit(rng.standard_normal((12, 768)).astype(np.float32))
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)
    assert tiles_a.max() < T1 <= tiles_b.min()
    assert float((emb @ u).min()) > 0.02                        # every cosine with -u is negative
    doc_off = np.arange(C + 1, dtype=np.int64)
    ix = mods["CorpusIndex"](doc_ids=np.arange(C, dtype=np.int64), doc_off=doc_off.astype(np.int32),
                             chunk_ids=np.arange(C, dtype=np.int64), emb=emb, total_docs=C)
    q = rng.standard_normal((300, 768)).astype(np.float32) * rng.uniform(0.5, 8, size=(300, 1)).astype(np.float32)
    q[6:40] = emb[rng.integers(0, C, 34)] + 0.4 * unit(q[6:40])
    q[Q_A] = va * 2.0                                           # every top-k document inside segment 1
    q[Q_B] = vb * 0.7                                           # ... inside segment 2
    q[Q_NEG] = -u * 3.0                                         # every cosine negative
    q[Q_NEG + 1] = -u * 0.2 + 1e-3 * unit(q[Q_NEG + 1:Q_NEG + 2])[0]
    q[Q_LAST] = emb[C - 1] * 0.8                                # the last row of the last, short tile
    q[130] = -u                                                 # (one more in the upper half of the batch)
    # a batch of queries that all look at group B: every top-k document in segment 2
    qb = (vb[None, :] * rng.uniform(0.5, 4, size=(256, 1)).astype(np.float32)
          + 0.05 * unit(rng.standard_normal((256, 768)).astype(np.float32))).astype(np.float32)
    q.setflags(write=False)
    qb.setflags(write=False)
    return dict(ix=ix, emb=emb, doc_off=doc_off, C=C, q=q, qb=qb, u=u, rows_a=rows_a, rows_b=rows_b)


@pytest.fixture(scope="module")
def engines(mods, corpus):
    made = {}

    def get(max_q, single, row_copy=True):
        key = (max_q, single, row_copy)
        if key not in made:
            made[key] = mods["DeviceEngine"](corpus["ix"], max_queries=max_q, max_k=100, rerank_max_docs=0,
                                             single_emit=single, row_copy=row_copy)
        return made[key]
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


def _equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


PICK = [Q_A, Q_B, Q_NEG, Q_NEG + 1, Q_LAST, 20, 130, 199, 255]


@pytest.mark.parametrize("max_q,Q,row_copy", [(256, 129, True), (256, 200, True), (256, 256, True), (512, 300, False)])
def test_segmented_and_single_emit_agree_and_match_the_oracle(mods, corpus, engines, max_q, Q, row_copy):
    """One group with (129, 200) and without (256) padding queries, and two groups in one launch over the f32 rows (300
    queries on a 512-query engine without row copies): the segmented and the one-launch engine return the same arrays bit
    for bit, both are the oracle's answer for a handful of queries (the negative ones among them), nobody fell back."""
    q = corpus["q"][:Q]
    seg_eng, one_eng = engines(max_q, False, row_copy), engines(max_q, True, row_copy)
    got = seg_eng.dense_topk(q, k=K)
    assert seg_eng.dense_path() == 256
    n_seg = _segmented_or_skip(seg_eng)
    ref = one_eng.dense_topk(q, k=K)
    seg1, n_one = one_eng.dense_pass_info()
    assert one_eng.dense_path() == 256 and seg1 == 1
    g, r = _np(got), _np(ref)
    assert _equal(g, r)
    assert bool((g[3] == K).all())                              # (nobody went back to the sweeps)
    pick = [i for i in PICK if i < Q]
    _check_dense(mods, seg_eng, corpus["doc_off"], corpus["emb"], q[pick], K, 0, [x[pick] for x in got])
    _check_dense(mods, one_eng, corpus["doc_off"], corpus["emb"], q[pick], K, 0, [x[pick] for x in ref])
    print(f"entries max_queries={max_q} Q={Q}: segmented {n_seg} single {n_one}")
    assert 0 < n_seg < n_one


def test_a_query_with_negative_scores_only(mods, corpus, engines):
    """-u against rows that all have a positive component along u: the top-k cosines, hence the thresholds and every tile
    maximum that matters, are negative."""
    q = corpus["q"][:256]
    best = -(corpus["emb"] @ corpus["u"])
    assert float(best.max()) < -0.02
    for single in (False, True):
        eng = engines(256, single)
        doc, score, chunk, n = _np(eng.dense_topk(q, k=K))
        if not single:
            _segmented_or_skip(eng)
        neg = [Q_NEG, Q_NEG + 1, 130]
        for i in neg:
            assert n[i] == K and np.all(score[i] < 0)
        _check_dense(mods, eng, corpus["doc_off"], corpus["emb"], q[neg], K, 0,
                     [torch.from_numpy(x[neg]) for x in (doc, score, chunk, n)])


def test_dense_begin_bounds_agree(corpus, engines):
    """dense_begin's per-query value is a function of the k_part-th largest tile maximum only.  The two engines emit
    different entries under different thresholds and must recover the same maxima: equal bit for bit, for k_part = k and
    ceil(k / 4); the outputs of dense_end as well."""
    q = corpus["q"][:256]
    eng, one = engines(256, False), engines(256, True)
    for k_part in (K, (K + 3) // 4):
        part = eng.dense_begin(q, k=K, k_part=k_part)
        n_seg = _segmented_or_skip(eng)
        part_ref = one.dense_begin(q, k=K, k_part=k_part)
        assert one.dense_pass_info()[0] == 1 and one.dense_pass_info()[1] > n_seg
        p, pr = part.cpu().numpy(), part_ref.cpu().numpy()
        assert np.array_equal(p.view(np.uint32), pr.view(np.uint32))
        assert np.all(np.isfinite(p)) and p[Q_NEG] < 0
        assert _equal(_np(eng.dense_end(256, k=K)), _np(one.dense_end(256, k=K)))


def test_the_raise_sees_the_maxima_of_segment_1(mods, corpus, engines):
    """256 queries whose top-k documents all lie in segment 2.  The segmented engine emits strictly fewer entries than the
    one-launch engine only if the raise between the segments read the right maxima of segment 1 (a row of -inf, or a short
    one, would leave every threshold where the sample put it)."""
    qb = corpus["qb"]
    eng, one = engines(256, False), engines(256, True)
    got = eng.dense_topk(qb, k=K)
    n_seg = _segmented_or_skip(eng)
    ref = one.dense_topk(qb, k=K)
    n_one = one.dense_pass_info()[1]
    g = _np(got)
    assert _equal(g, _np(ref))
    assert g[0].min() >= T1 * 256 and set(g[0][0].tolist()) <= set(corpus["rows_b"].tolist())
    _check_dense(mods, eng, corpus["doc_off"], corpus["emb"], qb[[0, 77, 255]], K, 0, [x[[0, 77, 255]] for x in got])
    print(f"entries, segment-2 batch: segmented {n_seg} single {n_one}")
    assert 0 < n_seg < n_one


def test_back_to_back_calls_equal_fresh_engines(mods, corpus, engines):
    """Two calls of different queries on one engine, the first with high tile maxima (group B), the second with the batch
    that holds the negative queries: each equals the same call on an engine that has seen nothing else.  Maxima left in the
    matrix by the first call would raise the second call's thresholds past its documents."""
    eng = engines(256, False)
    first = _np(eng.dense_topk(corpus["qb"], k=K))
    second = _np(eng.dense_topk(corpus["q"][:200], k=K))
    _segmented_or_skip(eng)
    n_second = eng.dense_pass_info()[1]
    for q, want, n_want in ((corpus["qb"], first, None), (corpus["q"][:200], second, n_second)):
        fresh = mods["DeviceEngine"](corpus["ix"], max_queries=256, max_k=100, rerank_max_docs=0)
        try:
            assert _equal(_np(fresh.dense_topk(q, k=K)), want)
            if n_want is not None:
                assert fresh.dense_pass_info()[1] == n_want     # the same thresholds: the same entries
        finally:
            fresh.close()
    assert bool((second[3] == K).all())
