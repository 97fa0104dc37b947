"""Removing documents on the GPU: msr_compact_postings against the CPU restatement (index_build.compact_postings) bit for
bit at tile edges and skewed shapes, its refusals, the whole remove_documents on cuda, and a live engine / Retriever
rebound to the shrunk or replaced index (Retriever.update_index) against fresh ones built from scratch."""
import ctypes as C

import numpy as np
import pytest
import torch

from index_cases import table
from msretr import _abi
from msretr.chunk_index import ChunkTable, attach_chunks
from msretr.index import DIM, _np
from msretr.index_build import bm25_add_token_ids, bm25_index_from_token_ids, compact_postings, remove_documents

pytestmark = pytest.mark.gpu
TILE = 2048                                                  # postings per workgroup of msr_compact.hip
TABLES = ("doc_ids", "doc_len", "term_off", "post_doc", "post_tf", "idf")


def check(t, keep):
    want = compact_postings(*t, keep)
    got = compact_postings(*t, keep, device="cuda")
    for g, w in zip(got, want):
        assert g.is_cuda and g.dtype == w.dtype and torch.equal(g.cpu(), w)
    return got


@pytest.mark.parametrize("P", [TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE + 3, 37 * TILE + 5])
def test_compact_tile_edges(P):
    rng = np.random.default_rng(P)
    t = table(rng, 3000, 900, P)
    assert int(t[0][-1]) == P
    for frac in (0.01, 0.3, 0.9):
        check(t, rng.random(3000) >= frac)


def test_compact_head_term_one_posting_terms_and_empty_terms():
    rng = np.random.default_rng(5)
    n = 600_000
    t = table(rng, n, 3000, 300_000, head=n)                 # term 0 spans ~290 tiles
    keep = rng.random(n) >= 0.01
    keep[1000:9000] = False                                  # and a block
    check(t, keep)
    many = table(rng, 200_000, 100_000, 100_000)             # ~10^5 one-posting terms
    assert np.median(np.diff(many[0])) == 1
    check(many, rng.random(200_000) >= 0.2)
    tail = table(rng, 5000, 4000, 40_000, empty_tail=700)    # trailing empty terms
    check(tail, rng.random(5000) >= 0.5)
    # terms emptied by the removal: every holder of the first 50 terms goes
    keep = np.ones(5000, bool)
    keep[np.unique(tail[1][:tail[0][50]])] = False
    got = check(tail, keep)
    assert int(got[0][50].item()) == 0


def test_compact_keep_all_and_keep_none():
    rng = np.random.default_rng(6)
    t = table(rng, 7000, 1500, 5 * TILE + 17)
    got = check(t, np.ones(7000, bool))
    assert np.array_equal(got[0].cpu().numpy(), t[0]) and np.array_equal(got[1].cpu().numpy(), t[1])
    got = check(t, np.zeros(7000, bool))
    assert got[1].numel() == 0 and not got[0].cpu().any()
    empty = (np.zeros(11, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32))
    check(empty, np.ones(4, bool))


def _raw_compact(t, keep, n_docs, capacity):
    """msr_compact_postings with caller-owned outputs pre-filled with -7 -> (rc, n_postings, term_off, post_doc, post_tf)."""
    lib = _abi.load()
    dev = torch.device("cuda")
    off = torch.as_tensor(t[0]).to(dev, torch.int64).contiguous()
    doc = torch.as_tensor(t[1]).to(dev, torch.int32).contiguous()
    tf = torch.as_tensor(t[2]).to(dev, torch.int32).contiguous()
    kp = torch.as_tensor(np.asarray(keep, np.uint8)).to(dev).contiguous()
    n_terms = len(t[0]) - 1
    out_off = torch.full((n_terms + 1,), -7, dtype=torch.int64, device=dev)
    out_doc = torch.full((max(capacity, 1),), -7, dtype=torch.int32, device=dev)
    out_tf = torch.full((max(capacity, 1),), -7, dtype=torch.int32, device=dev)
    n = C.c_int64(-1)
    p = lambda x: C.c_void_p(x.data_ptr()) if x.numel() else C.c_void_p(0)
    rc = lib.msr_compact_postings(p(off), n_terms, p(doc), p(tf), p(kp), n_docs, p(out_off), p(out_doc), p(out_tf), capacity,
                                  C.byref(n), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, n.value, out_off.cpu(), out_doc.cpu(), out_tf.cpu()


def test_compact_refusals_leave_the_output_untouched():
    rng = np.random.default_rng(3)
    t = table(rng, 20_000, 800, 90_000)
    keep = rng.random(20_000) >= 0.1
    K = int(keep[t[1]].sum())
    untouched = lambda r: all(bool((x == -7).all()) for x in r[2:])
    bad_off = t[0].copy()
    bad_off[100] = bad_off[101] + 1                          # not monotone
    r = _raw_compact((bad_off, t[1], t[2]), keep, 20_000, K)
    assert r[0] == -1 and untouched(r)
    bad_doc = t[1].copy()
    bad_doc[77_777] = 20_000                                 # outside [0, n_docs)
    r = _raw_compact((t[0], bad_doc, t[2]), keep, 20_000, K)
    assert r[0] == -1 and untouched(r)
    bad_doc[77_777] = -3
    r = _raw_compact((t[0], bad_doc, t[2]), keep, 20_000, K)
    assert r[0] == -1 and untouched(r)
    r = _raw_compact(t, keep, 20_000, K - 1)                 # capacity below the count
    assert r[0] == -1 and r[1] == K and untouched(r)
    r = _raw_compact(t, keep, 20_000, 0)                     # the sizing call writes nothing
    assert r[0] == 0 and r[1] == K and untouched(r)
    r = _raw_compact(t, keep, 20_000, K)                     # and the well-formed call succeeds
    want = compact_postings(*t, keep)
    assert r[0] == 0 and r[1] == K and torch.equal(r[2], want[0]) and torch.equal(r[3][:K], want[1])


def token_batch(rng, ids, n_terms, max_len=120):
    lens = rng.integers(1, max_len, len(ids))
    lens[rng.random(len(ids)) < 0.05] = 0
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return np.asarray(ids, np.int64), off, ((rng.zipf(1.2, int(off[-1])) - 1) % n_terms).astype(np.int32)


def subset(b, keep):
    ids, off, tok = b
    idx = np.nonzero(keep)[0]
    lens = np.diff(off)[idx]
    src = np.repeat(off[idx] - np.concatenate([[0], np.cumsum(lens)[:-1]]), lens) + np.arange(int(lens.sum()))
    return ids[idx], np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), tok[src]


def concat(batches):
    ids = np.concatenate([b[0] for b in batches])
    off = np.concatenate([[0], np.cumsum(np.concatenate([np.diff(b[1]) for b in batches]))]).astype(np.int64)
    return ids, off, np.concatenate([b[2] for b in batches])


def same_tables(got, want):
    for name in TABLES:
        g, w = np.asarray(_np(getattr(got, name))), np.asarray(_np(getattr(want, name)))
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), name
    assert np.float32(got.avgdl).tobytes() == np.float32(want.avgdl).tobytes() and got.total_docs == want.total_docs


def removal(rng, ids, pattern, frac):
    n = len(ids)
    if pattern == "scattered":
        return rng.choice(ids, int(n * frac), replace=False)
    s = int(rng.integers(0, n - int(n * frac)))
    return ids[s:s + int(n * frac)]


@pytest.mark.parametrize("pattern", ["scattered", "block"])
def test_whole_remove_on_cuda(pattern):
    rng = np.random.default_rng(11 if pattern == "scattered" else 12)
    ids = np.sort(rng.choice(900_000, 30_000, replace=False)).astype(np.int64) + 1
    b = token_batch(rng, ids, 20_000)
    ix_gpu = bm25_index_from_token_ids(*b, 20_000, device="cuda")
    ix_cpu = bm25_index_from_token_ids(*b, 20_000)
    R = removal(rng, np.asarray(ix_gpu.doc_ids), pattern, 0.05)
    new_gpu = remove_documents(ix_gpu, R, device="cuda")
    assert new_gpu.post_doc.is_cuda and new_gpu.update_counts["removed"] == len(R)
    same_tables(new_gpu, remove_documents(ix_cpu, R))
    same_tables(new_gpu, bm25_index_from_token_ids(*subset(b, ~np.isin(b[0], R)), 20_000, device="cuda"))


# ---------------------------------------------------------------------------------------------------------------- live engine
def chunks(rng, doc_ids, first):
    per = rng.integers(1, 5, len(doc_ids))
    own = np.repeat(np.asarray(doc_ids, np.int64), per)
    e = rng.standard_normal((len(own), DIM)).astype(np.float32)
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    return ChunkTable(chunk_ids=np.arange(first, first + len(own), dtype=np.int64), doc_ids=own, seqs=[[1]] * len(own),
                      emb=torch.as_tensor(e))


def drop(t, gone):
    k = ~np.isin(t.doc_ids, gone)
    return ChunkTable(chunk_ids=t.chunk_ids[k], doc_ids=t.doc_ids[k], seqs=[s for s, x in zip(t.seqs, k) if x],
                      emb=t.emb[torch.as_tensor(k)])


def meta(ids, tag=""):
    return {int(d): (f"http://s{int(d) % 13}.org/{tag}d{int(d)}", f"T{tag}{int(d)}", f"text {tag}of {int(d)}") for d in ids}


def with_urls(ix, m):
    ix.urls, ix.titles, ix.texts = [[m[int(d)][j] for d in ix.doc_ids] for j in range(3)]
    return ix


def corpus(seed):
    rng = np.random.default_rng(seed)
    ids = np.sort(rng.choice(300_000, 9000, replace=False)).astype(np.int64) + 1
    b0 = token_batch(rng, ids, 6000)
    k0 = b0[0][np.diff(b0[1]) > 0]
    t0 = chunks(rng, np.sort(k0), 0)
    m0 = meta(ids)
    base = with_urls(attach_chunks(bm25_index_from_token_ids(*b0, 6000), t0), m0)
    return rng, b0, t0, m0, base


def queries(rng, ix, rows_emb, n):
    """Term lists over frequent terms, and query vectors near the given chunk rows."""
    df = np.diff(np.asarray(_np(ix.term_off)))
    top = np.argsort(-df)[:400]
    terms = [rng.choice(top, rng.integers(1, 5)).tolist() for _ in range(n)]
    rows = rng.choice(len(rows_emb), n)
    qv = rows_emb[rows].numpy() + 0.05 * rng.standard_normal((n, DIM)).astype(np.float32)
    return terms, qv, rows


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b) if x is not None)


def warm(r, terms, qv):
    eng = r.engine
    eng.enable_bf16()
    eng.bm25_topk(terms[:8], k=100)
    eng.dense_topk(qv[:8], k=10)
    r.quick_search_batch(query_embeddings=qv[:4], top_k=10)
    r.quick_search_batch(query_embeddings=qv[:4], top_k=10, return_unique_docs=False)
    r.search_batch(["q"] * 4, top_k=100, query_embeddings=qv[:4], term_lists=terms[:4])
    r.batch_search([(i, "q") for i in range(4)], query_embeddings=qv[:4], term_lists=terms[:4]).text()


def compare(r, fresh, terms, qv, ix):
    """Every path of the rebound retriever equals the fresh one; returns the doc ids the dense paths returned."""
    eng, fe = r.engine, fresh.engine
    assert eng.row_copy_state() == fe.row_copy_state()
    assert same(eng.bm25_topk(terms, k=100), fe.bm25_topk(terms, k=100))
    served = []
    for kw in ({}, {"max_chunks_per_doc": 2}):
        got = eng.dense_topk(qv, k=10, **kw)
        assert same(got, fe.dense_topk(qv, k=10, **kw))
        served.append(got[0][got[0] >= 0].cpu().numpy())
    got = eng.dense_topk_batched(qv[:200], k=10)
    assert same(got, fe.dense_topk_batched(qv[:200], k=10))
    served.append(got[0][got[0] >= 0].cpu().numpy())
    ids = np.asarray(ix.doc_ids)
    out = set(ids[np.concatenate(served)].tolist())
    sb = r.search_batch(["q"] * 16, top_k=100, query_embeddings=qv[:16], term_lists=terms[:16])
    assert sb == fresh.search_batch(["q"] * 16, top_k=100, query_embeddings=qv[:16], term_lists=terms[:16])
    lines = lambda rt: rt.batch_search([(i, "q") for i in range(16)], query_embeddings=qv[:16], term_lists=terms[:16]).text()
    assert lines(r) == lines(fresh)
    for unique in (True, False):
        got = r.quick_search_batch(query_embeddings=qv[:8], top_k=10, return_unique_docs=unique)
        assert got == fresh.quick_search_batch(query_embeddings=qv[:8], top_k=10, return_unique_docs=unique)
        out |= {int(row["doc_id"]) for rows in got for row in rows}
    return out


@pytest.mark.parametrize("row_copy", [True, False])
def test_removed_documents_leave_the_live_engine(row_copy):
    from msretr.retriever import Retriever
    rng, b0, t0, m0, base = corpus(31)
    R = removal(rng, np.asarray(base.doc_ids), "scattered", 0.1)
    R = np.concatenate([R, removal(rng, np.setdiff1d(np.asarray(base.doc_ids), R), "block", 0.05)])
    removed = remove_documents(base, R)
    scratch = with_urls(attach_chunks(bm25_index_from_token_ids(*subset(b0, ~np.isin(b0[0], R)), 6000), drop(t0, R)), m0)
    gone = torch.as_tensor(np.isin(t0.doc_ids, R))
    terms, qv, _ = queries(rng, base, t0.emb[gone], 300)     # near the removed documents' chunks
    r = Retriever(indexer=base, max_queries=256, row_copy=row_copy)
    warm(r, terms, qv)
    r.update_index(removed)
    fresh = Retriever(indexer=scratch, max_queries=256, row_copy=row_copy)
    fresh.engine.enable_bf16()
    served = compare(r, fresh, terms, qv, removed)
    assert served and not served & set(R.tolist())
    assert r.bm25.index is removed and r.reranker.index is removed
    fresh.engine.close()
    r.engine.close()


def test_replaced_documents_on_the_live_engine():
    from msretr.retriever import Retriever
    rng, b0, t0, m0, base = corpus(32)
    R = removal(rng, np.asarray(base.doc_ids), "scattered", 0.05)
    rb = token_batch(rng, np.sort(R), 6500)
    rb = subset(rb, np.diff(rb[1]) > 0)
    m1 = meta(R, "v2/")
    t1 = chunks(rng, rb[0], int(t0.chunk_ids.max()) + 1)
    r = Retriever(indexer=base, max_queries=256)
    terms, qv, rows = queries(rng, base, t1.emb, 300)        # near the NEW versions' chunks
    warm(r, terms, qv)
    grown = bm25_add_token_ids(remove_documents(base, R), *rb, 6500, docs_meta=m1)
    assert grown.update_counts["already_indexed"] == 0
    r.update_index(attach_chunks(grown, t1))
    final = with_urls(attach_chunks(bm25_index_from_token_ids(*concat([subset(b0, ~np.isin(b0[0], R)), rb]), 6500),
                                    drop(t0, R), t1), m0 | m1)
    same_tables(grown, final)
    fresh = Retriever(indexer=final, max_queries=256)
    fresh.engine.enable_bf16()
    compare(r, fresh, terms, qv, grown)
    top1 = np.asarray(grown.doc_ids)[r.engine.dense_topk(qv, k=10)[0][:, 0].cpu().numpy()]
    assert np.mean(top1 == t1.doc_ids[rows]) > 0.9           # the replaced documents are found by their new text
    assert grown.urls == final.urls
    fresh.engine.close()
    r.engine.close()
