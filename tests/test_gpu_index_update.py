"""Index update on the GPU: msr_merge_postings against the CPU restatement bit for bit, its refusals, the whole
bm25_add_token_ids on cuda, and a live engine / Retriever rebound to the grown index (DeviceEngine.rebind,
Retriever.update_index) against fresh ones built on the from-scratch union."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from index_cases import maps, side
from msretr import _abi
from msretr.chunk_index import ChunkTable, attach_chunks
from msretr.engine import DeviceEngine, _ptr
from msretr.index import DIM, _np
from msretr.index_build import bm25_add_token_ids, bm25_index_from_token_ids, merge_postings

pytestmark = pytest.mark.gpu
TILE = 2048                                                  # outputs per workgroup of msr_merge.hip
TABLES = ("doc_ids", "doc_len", "term_off", "post_doc", "post_tf", "idf")


def check_merge(a, a_map, b, b_map, n_terms, n_docs, a_docs):
    want = merge_postings(*a, a_map, *b, b_map, n_terms, n_docs, a_docs=a_docs)
    got = merge_postings(*a, a_map, *b, b_map, n_terms, n_docs, device="cuda", a_docs=a_docs)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and torch.equal(g.cpu(), w)


@pytest.mark.parametrize("pattern", ["appended", "interleaved"])
def test_merge_head_term_and_one_sided_terms(pattern):
    rng = np.random.default_rng(1 if pattern == "appended" else 2)
    na, nb, V = 1_050_000, 12_000, 3000
    a = side(rng, na, V, 400_000, head=na)                   # term 0: every A document (>= 1e6 postings with B's)
    b = side(rng, nb, V + 200, 60_000, head=nb)              # terms V .. V+199: new terms, B only
    # terms only on the A side: drop B's postings of terms 1 .. 99
    keep = np.ones(len(b[1]), bool)
    keep[b[0][1]:b[0][100]] = False
    cnt = np.diff(b[0]); cnt[1:100] = 0
    b = (np.concatenate([[0], np.cumsum(cnt)]), b[1][keep], b[2][keep])
    a_map, b_map = maps(rng, na, nb, pattern)
    check_merge(a, a_map, b, b_map, V + 300, na + nb, na)


@pytest.mark.parametrize("P", [TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1, 37 * TILE + 5])
@pytest.mark.parametrize("pattern", ["appended", "interleaved"])
def test_merge_tile_edges(P, pattern):
    rng = np.random.default_rng(P)
    na, nb, V = 3000, 400, 1200
    pb = P // 5
    a, b = side(rng, na, V, P - pb), side(rng, nb, V, pb)
    assert int(a[0][-1]) + int(b[0][-1]) == P
    a_map, b_map = maps(rng, na, nb, pattern)
    check_merge(a, a_map, b, b_map, V, na + nb, na)


def test_merge_many_one_posting_terms_new_terms_only_and_empty_update():
    rng = np.random.default_rng(7)
    na, V = 5000, 200_000
    a = side(rng, na, V, 150_000)                            # mostly one-posting terms
    b = side(rng, 300, V + 50_000, 40_000, first_term=V)     # new terms only
    a_map, b_map = maps(rng, na, 300, "interleaved")
    check_merge(a, a_map, b, b_map, V + 50_000, na + 300, na)
    empty = (np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32))
    check_merge(a, None, empty, np.zeros(0, np.int32), V, na, na)


def _raw_merge(a, a_map, a_docs, b, b_map, n_terms, n_docs, capacity):
    """msr_merge_postings with caller-owned outputs pre-filled with -7 -> (rc, term_off, post_doc, post_tf)."""
    lib = _abi.load()
    dev = torch.device("cuda")
    t = lambda x, dt: None if x is None else torch.as_tensor(np.asarray(x)).to(dev, dt).contiguous()
    ao, ad, at = t(a[0], torch.int64), t(a[1], torch.int32), t(a[2], torch.int32)
    bo, bd, bt = t(b[0], torch.int64), t(b[1], torch.int32), t(b[2], torch.int32)
    am, bm = t(a_map, torch.int32), t(b_map, torch.int32)
    term_off = torch.full((n_terms + 1,), -7, dtype=torch.int64, device=dev)
    post_doc = torch.full((max(capacity, 1),), -7, dtype=torch.int32, device=dev)
    post_tf = torch.full((max(capacity, 1),), -7, dtype=torch.int32, device=dev)
    p = lambda x: C.c_void_p(x.data_ptr()) if x is not None and x.numel() else C.c_void_p(0)
    rc = lib.msr_merge_postings(p(ao), len(a[0]) - 1, p(ad), p(at), p(am), a_docs, p(bo), len(b[0]) - 1, p(bd), p(bt), p(bm),
                                0 if b_map is None else len(b_map), n_terms, n_docs, p(term_off), p(post_doc), p(post_tf),
                                capacity, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, term_off.cpu(), post_doc.cpu(), post_tf.cpu()


def test_merge_refusals_leave_the_output_untouched():
    rng = np.random.default_rng(3)
    na, nb, V = 20_000, 500, 800
    a, b = side(rng, na, V, 90_000), side(rng, nb, V, 3000)
    P = int(a[0][-1] + b[0][-1])
    b_map = np.arange(na, na + nb, dtype=np.int32)
    untouched = lambda r: all(bool((x == -7).all()) for x in r[1:])
    # a B document mapped onto an A document that has a posting of the same term: a clash
    t = int(np.nonzero(np.diff(a[0]))[0][0])
    x = int(a[1][a[0][t]])
    one = (np.concatenate([np.zeros(t + 1, np.int64), np.ones(V - t, np.int64)]), np.zeros(1, np.int32), np.ones(1, np.int32))
    r = _raw_merge(a, None, na, one, np.array([x], np.int32), V, na, int(a[0][-1]) + 1)
    assert r[0] == -1 and untouched(r)
    bad_map = b_map.copy()
    bad_map[[3, 4]] = bad_map[[4, 3]]
    r = _raw_merge(a, None, na, b, bad_map, V, na + nb, P)
    assert r[0] == -1 and untouched(r)
    r = _raw_merge(a, None, na, b, b_map, V, na + nb, P - 1)
    assert r[0] == -1 and untouched(r)
    r = _raw_merge(a, None, na, b, b_map, V, na + nb, P)     # and the well-formed call succeeds
    assert r[0] == 0 and int(r[1][-1]) == P
    # documents on both sides WITHOUT a shared term (the urlsDB-only documents of an update) are no clash
    shared = np.setdiff1d(np.arange(na), np.unique(a[1]))[:5]
    if len(shared):
        bs = side(rng, len(shared), V, 40)
        r = _raw_merge(a, None, na, bs, shared.astype(np.int32), V, na, int(a[0][-1] + bs[0][-1]))
        assert r[0] == 0


def token_batch(rng, ids, n_terms, max_len=120):
    lens = rng.integers(1, max_len, len(ids))
    lens[rng.random(len(ids)) < 0.05] = 0
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return np.asarray(ids, np.int64), off, ((rng.zipf(1.2, int(off[-1])) - 1) % n_terms).astype(np.int32)


def concat(batches):
    ids = np.concatenate([b[0] for b in batches])
    off = np.concatenate([[0], np.cumsum(np.concatenate([np.diff(b[1]) for b in batches]))]).astype(np.int64)
    return ids, off, np.concatenate([b[2] for b in batches])


def split(rng, n, pattern):
    ids = np.sort(rng.choice(30 * n, n, replace=False)).astype(np.int64) + 1
    if pattern == "appended":
        return ids[: n * 9 // 10], ids[n * 9 // 10:]
    upd = rng.random(n) < 0.1
    return ids[~upd], rng.permutation(ids[upd])


def same_tables(got, want):
    for name in TABLES:
        g, w = np.asarray(_np(getattr(got, name))), np.asarray(_np(getattr(want, name)))
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), name
    assert np.float32(got.avgdl) == np.float32(want.avgdl) and got.total_docs == want.total_docs


@pytest.mark.parametrize("pattern", ["appended", "interleaved"])
def test_whole_update_on_cuda(pattern):
    rng = np.random.default_rng(11)
    g0, g1 = split(rng, 30_000, pattern)
    b0, b1 = token_batch(rng, g0, 20_000), token_batch(rng, g1, 24_000)
    ix_gpu = bm25_index_from_token_ids(*b0, 20_000, device="cuda")
    ix_cpu = bm25_index_from_token_ids(*b0, 20_000)
    new_gpu = bm25_add_token_ids(ix_gpu, *b1, 24_000, device="cuda")
    assert new_gpu.post_doc.is_cuda
    same_tables(new_gpu, bm25_add_token_ids(ix_cpu, *b1, 24_000))
    same_tables(new_gpu, bm25_index_from_token_ids(*concat([b0, b1]), 24_000, device="cuda"))


# ---------------------------------------------------------------------------------------------------------------- live engine
def chunks(rng, doc_ids, first):
    per = rng.integers(1, 5, len(doc_ids))
    own = np.repeat(np.asarray(doc_ids, np.int64), per)
    e = rng.standard_normal((len(own), DIM)).astype(np.float32)
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    return ChunkTable(chunk_ids=np.arange(first, first + len(own), dtype=np.int64), doc_ids=own, seqs=[[1]] * len(own),
                      emb=torch.as_tensor(e))


def corpus(pattern):
    """base index, the grown one (update + chunks of the new documents) and the from-scratch union."""
    rng = np.random.default_rng(21 if pattern == "appended" else 22)
    g0, g1 = split(rng, 9000, pattern)
    b0, b1 = token_batch(rng, g0, 6000), token_batch(rng, g1, 6500)
    k0 = b0[0][np.diff(b0[1]) > 0]
    k1 = b1[0][np.diff(b1[1]) > 0]
    t0 = chunks(rng, np.sort(k0), 0)
    t1 = chunks(rng, np.sort(k1), t0.next_chunk_id)
    meta = lambda ids: {int(d): (f"http://s{int(d) % 13}.org/d{int(d)}", f"T{int(d)}", f"text of {int(d)}") for d in ids}
    base = attach_chunks(bm25_index_from_token_ids(*b0, 6000), t0)
    m0 = meta(base.doc_ids)
    base.urls, base.titles, base.texts = [[m0[int(d)][j] for d in base.doc_ids] for j in range(3)]
    grown = attach_chunks(bm25_add_token_ids(base, *b1, 6500, docs_meta=meta(g1)), t1)
    union = attach_chunks(bm25_index_from_token_ids(*concat([b0, b1]), 6500), t0, t1)
    mu = meta(union.doc_ids)
    union.urls, union.titles, union.texts = [[mu[int(d)][j] for d in union.doc_ids] for j in range(3)]
    return base, grown, union, t1, rng


def queries(rng, ix, t1, n):
    """Term lists over frequent terms, and query vectors near chunks of the NEW documents (so they must be found)."""
    df = np.diff(np.asarray(_np(ix.term_off)))
    top = np.argsort(-df)[:400]
    terms = [rng.choice(top, rng.integers(1, 5)).tolist() for _ in range(n)]
    rows = rng.choice(len(t1), n)
    qv = t1.emb[rows].numpy() + 0.05 * rng.standard_normal((n, DIM)).astype(np.float32)
    return terms, qv, t1.doc_ids[rows]


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b) if x is not None)


@pytest.mark.parametrize("row_copy", [True, False])
@pytest.mark.parametrize("pattern", ["appended", "interleaved"])
def test_rebound_engine_equals_fresh_engine(pattern, row_copy):
    from msretr.retriever import Retriever
    base, grown, union, t1, rng = corpus(pattern)
    terms, qv, want_doc = queries(rng, union, t1, 300)
    r = Retriever(indexer=base, max_queries=256, row_copy=row_copy)
    eng = r.engine
    eng.enable_bf16()
    eng.bm25_topk(terms[:8], k=100)
    eng.dense_topk(qv[:8], k=10)
    r.quick_search_batch(query_embeddings=qv[:4], top_k=10)
    r.quick_search_batch(query_embeddings=qv[:4], top_k=10, return_unique_docs=False)
    r.search_batch(["q"] * 4, top_k=100, query_embeddings=qv[:4], term_lists=terms[:4])
    r.batch_search([(i, "q") for i in range(4)], query_embeddings=qv[:4], term_lists=terms[:4]).text()
    r.update_index(grown)
    fresh = Retriever(indexer=union, max_queries=256, row_copy=row_copy)
    fresh.engine.enable_bf16()
    assert eng.row_copy_state() == fresh.engine.row_copy_state()
    assert same(eng.bm25_topk(terms, k=100), fresh.engine.bm25_topk(terms, k=100))
    for kw in ({}, {"max_chunks_per_doc": 2}):
        assert same(eng.dense_topk(qv, k=10, **kw), fresh.engine.dense_topk(qv, k=10, **kw))
    d_new = eng.dense_topk_batched(qv[:200], k=10)
    assert same(d_new, fresh.engine.dense_topk_batched(qv[:200], k=10))
    top1 = np.asarray(grown.doc_ids)[d_new[0][:, 0].cpu().numpy()]
    assert np.mean(top1 == want_doc[:200]) > 0.9                 # the new documents are served
    assert r.search_batch(["q"] * 16, top_k=100, query_embeddings=qv[:16], term_lists=terms[:16]) == \
        fresh.search_batch(["q"] * 16, top_k=100, query_embeddings=qv[:16], term_lists=terms[:16])
    lines = lambda rt: rt.batch_search([(i, "q") for i in range(16)], query_embeddings=qv[:16], term_lists=terms[:16]).text()
    assert lines(r) == lines(fresh)
    for unique in (True, False):
        got = r.quick_search_batch(query_embeddings=qv[:8], top_k=10, return_unique_docs=unique)
        assert got == fresh.quick_search_batch(query_embeddings=qv[:8], top_k=10, return_unique_docs=unique)
        assert {row["doc_id"] for row in got[0]} & set(np.asarray(t1.doc_ids).tolist())
    assert r.bm25.index is grown and r.reranker.index is grown
    fresh.engine.close()
    eng.close()


def test_rebind_between_split_halves_and_failed_rebind():
    base, grown, union, t1, rng = corpus("appended")
    _, qv, _ = queries(rng, union, t1, 100)
    eng = DeviceEngine(base, max_queries=256)
    assert eng.dense_split_max(10) >= 100
    eng.dense_begin(qv, k=10)
    eng.rebind(grown)
    with pytest.raises(_abi.MsrError) as ei:
        eng.dense_end(100, k=10)
    assert ei.value.code == -1                                # MSR_ERR_INVALID: the begin was cancelled
    eng.dense_topk(qv, k=10)                                  # the engine serves the new index
    bad = bm25_index_from_token_ids(*token_batch(rng, np.arange(50), 40), 40)
    pd = np.asarray(_np(bad.post_doc)).copy()
    t = int(np.argmax(np.diff(np.asarray(_np(bad.term_off)))))
    o = np.asarray(_np(bad.term_off))
    pd[o[t]:o[t + 1]] = pd[o[t]:o[t + 1]][::-1].copy()       # documents descending inside a term: malformed
    bad.post_doc = pd
    with pytest.raises(_abi.MsrError):
        eng.rebind(bad)
    for call in (lambda: eng.bm25_topk([[1, 2]], k=10), lambda: eng.dense_topk(qv[:2], k=10)):
        with pytest.raises(_abi.MsrError) as ei:
            call()
        assert ei.value.code == -2                            # MSR_ERR_NOT_BOUND
    eng.rebind(union)
    assert eng.dense_topk(qv[:2], k=10)[3].cpu().tolist() == [10, 10]
    eng.close()


# ------------------------------------------------------------------------------- what the engine owns, and what is bound
@functools.lru_cache(maxsize=None)
def appended():
    """corpus("appended") built once for the tests below, and 100 query vectors near chunks of its new documents."""
    base, grown, union, t1, rng = corpus("appended")
    return base, grown, queries(rng, union, t1, 100)[1]


@pytest.mark.parametrize("bf16", [False, True])
def test_owned_bytes_after_unbind_and_rebind(bf16):
    """msr_owned_bytes as the ledger of the engine's lifetime groups: a second msr_unbind frees nothing more, and an engine
    re-bound to an index owns exactly what a fresh engine on that index owns."""
    base, grown, qv = appended()
    eng = DeviceEngine(base, max_queries=256)
    if bf16:
        eng.enable_bf16()
    built = eng.owned_bytes()
    eng.dense_topk(qv, k=10)
    eng.rebind(grown)
    fresh = DeviceEngine(grown, max_queries=256)
    if bf16:
        fresh.enable_bf16()
    assert eng.owned_bytes() == fresh.owned_bytes()
    assert same(eng.dense_topk(qv, k=10), fresh.dense_topk(qv, k=10))
    fresh.close()
    torch.cuda.synchronize()
    eng._check(eng.lib.msr_unbind(eng.handle))
    unbound = eng.owned_bytes()
    assert 0 < unbound < built
    eng._check(eng.lib.msr_unbind(eng.handle))
    assert eng.owned_bytes() == unbound
    eng.rebind(base)
    assert eng.owned_bytes() == built
    eng.close()


def test_raw_rebind_cancels_a_pending_begin():
    """msr_bind_chunks through the C ABI between the two halves of a split dense call, without an msr_unbind: the bind drops the
    old binding with its pending begin, so the end is refused (it would read the freed scratch of the pass) and the engine
    serves the new binding like a fresh one."""
    base, _, qv = appended()
    eng = DeviceEngine(base, max_queries=256)
    assert eng.dense_split_max(10) >= 100
    eng.dense_begin(qv, k=10)
    torch.cuda.synchronize()
    t = eng._t
    eng._check(eng.lib.msr_bind_chunks(eng.handle, _ptr(t["emb"]), int(t["emb"].shape[0]), _ptr(t["doc_off"]), base.n_docs,
                                       _ptr(t["inv_norm"]), eng._stream()))
    with pytest.raises(_abi.MsrError) as ei:
        eng.dense_end(100, k=10)
    assert ei.value.code == -1                                # MSR_ERR_INVALID: no matching begin
    fresh = DeviceEngine(base, max_queries=256)
    assert eng.owned_bytes() == fresh.owned_bytes()
    assert same(eng.dense_topk(qv, k=10), fresh.dense_topk(qv, k=10))
    fresh.close()
    eng.close()


def test_batched_call_is_refused_while_a_begin_is_pending():
    base, _, qv = appended()
    eng = DeviceEngine(base, max_queries=256)
    eng.enable_bf16()
    want = eng.dense_topk(qv, k=10)
    eng.dense_begin(qv, k=10)
    with pytest.raises(_abi.MsrError) as ei:
        eng.dense_topk_batched(qv, k=10)
    assert ei.value.code == -1                                # MSR_ERR_INVALID: the two share scratch
    assert same(eng.dense_end(100, k=10), want)                # the pending call is intact
    eng.close()
