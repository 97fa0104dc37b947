"""Every dense entry point against a float64 top-k of adversarially rounded corpora (tests/dense_adversary.py).

The corpora put each filter within ~0.15 of its margin (f16) and ~0.03 (bf16) -- test_dense_adversary.py shows on the CPU
that a filter with half the margin, a split bound with margin_scale 1/4 or an unmargined pass-1 threshold loses documents
on them.  Here the kernels must return the float64 answer: documents in order (the corpus keeps neighbouring exact
scores >= 2e-5 apart), every score within a bar derived from the f32 arithmetic of the kernel that produced it, the
first arg-max row, exact ties in ascending index with identical score bits.  Every case asserts the path that served it."""
import numpy as np
import pytest

import dense_adversary as A

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SWEEP_BAR = 8e-6            # f16x2 K-split / narrow sweeps: the proven bound


def rescore_bar(A_sum, s):
    """f32 rescore (msr_batch_rescore_rows, best_chunk_kernel): 12 products per lane + a 6-level shuffle tree (depth 18,
    counted 24) times inv_norm (its own depth-18 sum, sqrtf, division: 4 more roundings of |s|)."""
    return A.U32 * (24.0 * A_sum + 4.0 * abs(s)) + 1e-9


def exact_f32_bar(A_sum, s):
    """Exact-f32 K-split instance (v_mfma_f32_16x16x4_f32 chains, partial tiles summed over the waves): depth counted 64."""
    return A.U32 * (64.0 * A_sum + 4.0 * abs(s)) + 1e-9


@pytest.fixture(scope="module")
def mods():
    from msretr.engine import DeviceEngine
    from msretr.index import CorpusIndex
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return dict(DeviceEngine=DeviceEngine, CorpusIndex=CorpusIndex)


@pytest.fixture(scope="module")
def c16():
    return A.build("f16")


@pytest.fixture(scope="module")
def cb16():
    return A.build("bf16")


def _index(mods, c, d0=0, d1=None):
    d1 = c.n_docs if d1 is None else d1
    off = c.doc_off[d0:d1 + 1] - c.doc_off[d0]
    r0, r1 = int(c.doc_off[d0]), int(c.doc_off[d1])
    return mods["CorpusIndex"](doc_ids=np.arange(d0, d1, dtype=np.int64), doc_off=off.astype(np.int32),
                               chunk_ids=np.arange(r0, r1, dtype=np.int64), emb=c.emb[r0:r1], total_docs=c.n_docs,
                               doc_base=d0, row_base=r0)


_REF = {}


def _ref(c, qi, k, mc=0):
    key = (id(c), qi, k, mc)
    if key not in _REF:
        best, arg, cos = A.doc_max64(c.emb, c.doc_off, c.queries[qi].q, mc)
        top = A.topk64(best, k)
        q64 = c.queries[qi].q.astype(np.float64)
        rows = c.emb[arg[top]].astype(np.float64)
        a_sum = (np.abs(rows) @ np.abs(q64)) / np.linalg.norm(rows, axis=1)
        _REF[key] = (top, best[top], arg[top], a_sum)
    return _REF[key]


def check(c, qidx, k, got, bar, mc=0, worst=None):
    """The sharp checker: counts, document ids in order, |score - f64| <= bar, arg-max row = the f64 first arg-max, exact
    ties (equal f64 scores) with identical score bits.  `worst` (list) receives the largest error as a fraction of the bar."""
    doc, score, chunk, n = [x.cpu().numpy() for x in got]
    assert len(doc) == len(qidx)
    for i, qi in enumerate(qidx):
        top, s64, arg, a_sum = _ref(c, qi, k, mc)
        assert n[i] == len(top), (i, qi)
        assert np.array_equal(doc[i, :n[i]], top), (i, qi, np.nonzero(doc[i, :n[i]] != top)[0][:5])
        b = np.array([bar(a, s) for a, s in zip(a_sum, s64)])
        err = np.abs(score[i, :n[i]].astype(np.float64) - s64)
        assert np.all(err <= b), (i, qi, float((err / b).max()))
        if worst is not None:
            worst.append(float((err / b).max()))
        if chunk is not None:
            assert np.array_equal(chunk[i, :n[i]].astype(np.int64), arg), (i, qi)
        tie = s64[1:] == s64[:-1]
        assert np.array_equal(score[i, 1:n[i]][tie].view(np.uint32), score[i, :n[i] - 1][tie].view(np.uint32))


def _batch(c, k, Q, kinds=("planted",), extra_k10=True):
    """Q queries cycling through the planted queries of this k (k = 10 also: the small twin group)."""
    idx = c.of_k(k, kinds=kinds + (("twins",) if (k == 10 and extra_k10) else ()))
    qidx = [idx[i % len(idx)] for i in range(Q)]
    return qidx, c.qmat(qidx)


# ------------------------------------------------------------------------------------------------ sweeps (<= 64 queries)
def test_f16x2_sweep_at_scores_near_one(mods, c16):
    """Q <= 64 on the default engine: the f16x2 K-split sweep.  Planted scores are ~0.997 ... 1 with one-signed products
    and lo pieces that are f16 subnormals: every score within the proven 8e-6 of float64 (this settles whether the matrix
    cores keep those pieces: dropped, the planted scores would be off by ~eps = 3.8e-4).  Also the narrow sweep
    (dense_scan_v2_kernel): max_chunks_per_doc = 1 and the interleaved layout."""
    eng = mods["DeviceEngine"](_index(mods, c16), max_queries=64, max_k=100, rerank_max_docs=0)
    assert eng.scan_arith() == "f16x2"
    worst = []
    for k in (1, 10, 100):
        qidx, q = _batch(c16, k, 40, kinds=("planted", "big"))
        check(c16, qidx, k, eng.dense_topk(q, k=k), lambda a, s: SWEEP_BAR, worst=worst)
        assert eng.dense_path() == 64
    qidx, q = _batch(c16, 10, 20)
    check(c16, qidx, 10, eng.dense_topk(q, k=10, max_chunks_per_doc=1), lambda a, s: SWEEP_BAR, mc=1)
    assert eng.dense_path() == 32
    eng.close()
    lay = mods["DeviceEngine"](_index(mods, c16), max_queries=32, max_k=100, rerank_max_docs=0, scan_layout=1)
    for k in (1, 10):
        qidx, q = _batch(c16, k, 24)
        check(c16, qidx, k, lay.dense_topk(q, k=k), lambda a, s: SWEEP_BAR, worst=worst)
        assert lay.dense_path() == 32
    lay.close()
    print(f"f16x2 sweeps: largest error {max(worst):.3f} of 8e-6")


def test_exact_f32_ksplit_instance(mods, c16):
    """scan_variant = 2: the exact-f32 K-split instance on the same corpus, the reference point (bar: the f32 FMA chain)."""
    eng = mods["DeviceEngine"](_index(mods, c16), max_queries=64, max_k=100, rerank_max_docs=0, scan_variant=2)
    assert eng.scan_arith() == "f32"
    worst = []
    for k in (1, 10, 100):
        qidx, q = _batch(c16, k, 64, kinds=("planted", "big"))
        check(c16, qidx, k, eng.dense_topk(q, k=k), exact_f32_bar, worst=worst)
    eng.close()
    print(f"exact f32 sweep: largest error {max(worst):.3f} of its bar")


# ------------------------------------------------------------------------------------------------ streaming passes
@pytest.mark.parametrize("k", (1, 10, 100))
def test_streaming_pass_128(mods, c16, k):
    """65 ... 128 queries: gemm_stream_kernel (f16 filter, exact f32 finish of the emitted rows).  k = 1 / 10 / 100 take
    sample strides 64 / 8 / 1."""
    eng = mods["DeviceEngine"](_index(mods, c16), max_queries=128, max_k=100, rerank_max_docs=0)
    assert eng.scan_width() == 128
    qidx, q = _batch(c16, k, 100)
    worst = []
    check(c16, qidx, k, eng.dense_topk(q, k=k), rescore_bar, worst=worst)
    assert eng.dense_path() == 128
    eng.close()
    print(f"stream128 k={k}: largest error {max(worst):.3f} of the rescore bar")


def test_streaming_pass_256(mods, c16):
    """129 ... 256 queries on a max_queries = 256 engine: gemm_stream256_kernel on the fragment-order copy of the f32 rows."""
    eng = mods["DeviceEngine"](_index(mods, c16), max_queries=256, max_k=100, rerank_max_docs=0)
    assert eng.row_copy_state() == "built"
    worst = []
    for k in (1, 10, 100):
        qidx, q = _batch(c16, k, 200)
        check(c16, qidx, k, eng.dense_topk(q, k=k), rescore_bar, worst=worst)
        assert eng.dense_path() == 256
    eng.close()
    print(f"stream256: largest error {max(worst):.3f} of the rescore bar")


def test_multi_group_launches_on_the_f16_image(mods, c16):
    """600 and 1000 queries on a max_queries = 1024 engine: launches of several 256-query groups on the f16 image of the
    rows; bit for bit what an engine without the image (row_copy=False: the f32 rows converted in registers) returns."""
    img = mods["DeviceEngine"](_index(mods, c16), max_queries=1024, max_k=100, rerank_max_docs=0)
    raw = mods["DeviceEngine"](_index(mods, c16), max_queries=1024, max_k=100, rerank_max_docs=0, row_copy=False)
    assert img.row_image_state() == "built" and raw.row_image_state() == "declined"
    for Q, k in ((600, 10), (1000, 100), (1000, 1)):
        qidx, q = _batch(c16, k, Q)
        a = img.dense_topk(q, k=k)
        assert img.dense_path() == 256
        check(c16, qidx, k, a, rescore_bar)
        b = raw.dense_topk(q, k=k)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    img.close()
    raw.close()


def test_big_twin_group_raises_only_its_slice_gate(mods, c16):
    """A query whose 5500 tied documents overflow the pass' candidate buffers (GF_PAIR_CAP = 4096): its 64-query slice goes
    to the gated sweeps (scores within 8e-6, ties by index), the other slice keeps the pass' answer -- bit for bit what the
    same batch without the twins query returns."""
    eng = mods["DeviceEngine"](_index(mods, c16), max_queries=128, max_k=100, rerank_max_docs=0)
    qidx, q = _batch(c16, 10, 100)
    big = c16.of_k(10, kinds=("big",))[0]
    with_big = list(qidx); with_big[5] = big
    got = eng.dense_topk(c16.qmat(with_big), k=10)
    assert eng.dense_path() == 128
    top = _ref(c16, big, 10)[0]
    assert np.all(np.diff(top) > 0)                                    # one exact tie group: ascending index
    lo = [x[:64] for x in got]
    check(c16, with_big[:64], 10, lo, lambda a, s: SWEEP_BAR)
    hi = [x[64:] for x in got]
    check(c16, with_big[64:], 10, hi, rescore_bar)
    plain = eng.dense_topk(q, k=10)
    assert all(torch.equal(x[64:], y[64:]) for x, y in zip(got, plain))
    check(c16, qidx, 10, plain, rescore_bar)
    eng.close()


# ------------------------------------------------------------------------------------------------ split call
@pytest.mark.parametrize("k", (1, 10))
def test_split_call_over_and_under_shards(mods, c16, k):
    """msr_dense_topk_begin / _end on two shard engines: A holds the over-documents, B the under-documents (and the twins).
    A's part (gemm_kth_kernel, margin_scale 0.5) is the bound; B raises its threshold with it (raise_thr_kernel).  The
    merged lists are the unsharded float64 top-k."""
    sd = c16.split_doc
    engs = [mods["DeviceEngine"](_index(mods, c16, 0, sd), max_queries=256, max_k=100, rerank_max_docs=0),
            mods["DeviceEngine"](_index(mods, c16, sd, c16.n_docs), max_queries=256, max_k=100, rerank_max_docs=0)]
    qidx, q = _batch(c16, k, 100)
    assert all(e.dense_split_max(k) >= 100 for e in engs)
    parts = [e.dense_begin(q, k=k, k_part=(k + 1) // 2) for e in engs]
    bound = torch.stack(parts).min(dim=0).values
    outs = [e.dense_end(100, k=k, bound=bound) for e in engs]
    base = [(0, 0), (sd, int(c16.doc_off[sd]))]
    glob = lambda t, b: torch.where(t >= 0, t + b, t)
    docs = torch.stack([glob(o[0], b[0]) for o, b in zip(outs, base)])
    m_doc, m_score, m_n = engs[0].merge_topk(docs, torch.stack([o[1] for o in outs]), torch.stack([o[3] for o in outs]), k)
    chunk = torch.full_like(m_doc, -1)
    for g, (o, b) in enumerate(zip(outs, base)):                       # the arg-max row travels with its document
        for i in range(100):
            for j in range(int(o[3][i])):
                hit = (m_doc[i] == int(docs[g, i, j])).nonzero()
                if len(hit):
                    chunk[i, hit[0, 0]] = int(o[2][i, j]) + b[1]
    check(c16, qidx, k, (m_doc, m_score, chunk, m_n), rescore_bar)
    for e in engs:
        e.close()


# ------------------------------------------------------------------------------------------------ batched bf16 path
def test_batched_bf16_paths(mods, cb16):
    """dense_topk_batched on the bf16 corpus: <= 128 queries = the bf16 K-split sweep + msr_batch_finish, > 128 queries =
    gemm_stream256_kernel<BF16> + msr_gemm.hip; k = 1 / 10 / 100.  The big twin group overflows MSR_SEL_CAP: out_n = -1
    and the host reruns that query on the f32 path -- still the float64 answer."""
    eng = mods["DeviceEngine"](_index(mods, cb16), max_queries=1024, max_k=100, rerank_max_docs=0)
    eng.enable_bf16()
    assert eng.batch_width() == 128 and eng.batch_gemm_ok()
    worst = []
    big = cb16.of_k(10, kinds=("big",))[0]
    for Q in (100, 300):
        for k in (1, 10, 100):
            qidx, q = _batch(cb16, k, Q)
            check(cb16, qidx, k, eng.dense_topk_batched(q, k=k), rescore_bar, worst=worst)
        qidx, _ = _batch(cb16, 10, Q)
        qidx[3] = big
        check(cb16, qidx[:3] + qidx[4:], 10, [x[torch.arange(Q) != 3] for x in eng.dense_topk_batched(cb16.qmat(qidx), k=10)],
              rescore_bar)
        got = eng.dense_topk_batched(cb16.qmat(qidx), k=10)
        top = _ref(cb16, big, 10)[0]
        assert got[0][3].cpu().numpy().tolist() == top.tolist() and int(got[3][3]) == 10
    eng.close()
    print(f"bf16 batched: largest error {max(worst):.3f} of the rescore bar")
