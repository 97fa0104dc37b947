"""Removing documents from a built index (index_build.remove_documents / compact_postings, CPU device): the tables must equal
a from-scratch build of the remaining documents bit for bit -- total_docs, avg_doc_length and the idf of every term move
with the removal -- and replace (remove, then add the new versions under the same ids) must equal a from-scratch build of
the final corpus, chunk side included."""
import numpy as np
import pytest
import torch

from msretr.chunk_index import ChunkTable, attach_chunks
from msretr.index import DIM, CorpusIndex, _np
from msretr.index_build import (bm25_add_token_ids, bm25_index_from_token_ids, compact_postings, idf_real,
                                remove_documents)

TABLES = ("doc_ids", "doc_len", "term_off", "post_doc", "post_tf", "idf")
CHUNK_SIDE = ("doc_off", "chunk_ids")


def batch(rng, ids, n_terms, empty_frac=0.15, max_len=40):
    """Token-id streams of documents `ids` (some without tokens), Zipf-like term ids below n_terms."""
    lens = rng.integers(1, max_len, len(ids))
    lens[rng.random(len(ids)) < empty_frac] = 0
    off = np.zeros(len(ids) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    tok = ((rng.zipf(1.3, int(off[-1])) - 1) % n_terms).astype(np.int32)
    return np.asarray(ids, np.int64), off, tok


def subset(b, keep):
    """The documents of batch b where keep is True, with their tokens."""
    ids, off, tok = b
    idx = np.nonzero(keep)[0]
    lens = np.diff(off)[idx]
    parts = [tok[off[i]:off[i + 1]] for i in idx]
    return ids[idx], np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), np.concatenate(parts + [np.zeros(0, np.int32)])


def concat(batches):
    ids = np.concatenate([b[0] for b in batches])
    off = np.concatenate([[0], np.cumsum(np.concatenate([np.diff(b[1]) for b in batches]))]).astype(np.int64)
    return ids, off, np.concatenate([b[2] for b in batches])


def assert_same_tables(got, want):
    for name in TABLES:
        g, w = np.asarray(_np(getattr(got, name))), np.asarray(_np(getattr(want, name)))
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), name
    assert np.float32(got.avgdl).tobytes() == np.float32(want.avgdl).tobytes()
    assert got.total_docs == want.total_docs and got.n_docs_global == got.n_docs


def assert_same_chunks(got, want):
    for name in CHUNK_SIDE:
        g, w = np.asarray(_np(getattr(got, name))), np.asarray(_np(getattr(want, name)))
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), name
    assert torch.equal(torch.as_tensor(got.emb).cpu(), torch.as_tensor(want.emb).cpu())


def snapshot(ix):
    names = TABLES + tuple(n for n in CHUNK_SIDE + ("emb",) if getattr(ix, n) is not None)
    return {n: np.asarray(_np(getattr(ix, n))).copy() for n in names}


def removal(rng, ids, pattern, frac=0.2):
    """The ids to remove: scattered, one contiguous block, or every other document."""
    n = len(ids)
    if pattern == "scattered":
        return rng.permutation(rng.choice(ids, max(1, int(n * frac)), replace=False))
    if pattern == "block":
        s = int(rng.integers(0, n - int(n * frac)))
        return ids[s:s + int(n * frac)]
    return ids[::2]


@pytest.mark.parametrize("pattern", ["scattered", "block", "alternate"])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_remove_equals_scratch_build(pattern, seed):
    rng = np.random.default_rng(50 * seed + len(pattern))
    V = int(rng.integers(150, 400))
    b = batch(rng, np.sort(rng.choice(10_000, 400, replace=False)).astype(np.int64) + 3, V)
    ix = bm25_index_from_token_ids(*b, V)
    R = removal(rng, np.asarray(ix.doc_ids), pattern)
    before = snapshot(ix)
    new = remove_documents(ix, R)
    for name, arr in before.items():                     # the old index is left as it was
        assert np.asarray(_np(getattr(ix, name))).tobytes() == arr.tobytes(), name
    want = bm25_index_from_token_ids(*subset(b, ~np.isin(b[0], R)), V)
    assert_same_tables(new, want)
    assert new.n_terms == ix.n_terms
    assert new.update_counts == dict(removed=len(R), removed_rows=len(R), not_found=0)
    # (a negative control: the idf must move with total_docs -- keeping the old idf of the surviving terms differs)
    assert np.asarray(_np(ix.idf)).tobytes() != np.asarray(_np(new.idf)).tobytes()


def test_remove_edge_cases():
    rng = np.random.default_rng(7)
    V = 60
    b = batch(rng, np.arange(300, dtype=np.int64) * 3 + 1, V, empty_frac=0.0)
    ix = bm25_index_from_token_ids(*b, V)
    ids = np.asarray(ix.doc_ids)
    # nothing
    new = remove_documents(ix, np.zeros(0, np.int64))
    assert_same_tables(new, ix)
    assert new.update_counts == dict(removed=0, removed_rows=0, not_found=0)
    # everything: shape-correct empty tables, equal to the empty from-scratch build
    new = remove_documents(ix, ids[::-1])
    empty = bm25_index_from_token_ids(np.zeros(0, np.int64), np.zeros(1, np.int64), np.zeros(0, np.int32), V)
    assert_same_tables(new, empty)
    assert new.n_docs == 0 and new.n_terms == V and new.total_docs == 0 and int(_np(new.term_off)[-1]) == 0
    # every holder of a term: the term stays in the vocabulary with no postings and the idf of df = 0
    off = np.asarray(_np(ix.term_off))
    df = np.diff(off)
    t = int(np.argmin(np.where(df > 0, df, len(ids) + 1)))      # the rarest term that has postings
    holders = ids[np.asarray(_np(ix.post_doc))[off[t]:off[t + 1]]]
    new = remove_documents(ix, holders)
    assert_same_tables(new, bm25_index_from_token_ids(*subset(b, ~np.isin(b[0], holders)), V))
    assert np.diff(np.asarray(_np(new.term_off)))[t] == 0
    assert np.asarray(_np(new.idf))[t] == idf_real(new.total_docs, [0])[0]
    # the last document
    new = remove_documents(ix, ids[-1:])
    assert_same_tables(new, bm25_index_from_token_ids(*subset(b, b[0] != ids[-1]), V))
    # ids the index does not have are counted
    new = remove_documents(ix, np.array([ids[5], 2, 10 ** 9, ids[0]], np.int64))
    assert new.update_counts == dict(removed=2, removed_rows=2, not_found=2)
    assert_same_tables(new, bm25_index_from_token_ids(*subset(b, ~np.isin(b[0], [ids[5], ids[0]])), V))
    # a duplicate id raises; a shard is refused
    with pytest.raises(ValueError, match="duplicate"):
        remove_documents(ix, np.array([ids[3], ids[3]]))
    for rank in (0, 1):
        with pytest.raises(ValueError, match="shard"):
            remove_documents(ix.shard(rank, 2), ids[:1])


def test_compact_postings_cpu():
    off = torch.tensor([0, 3, 3, 5, 6], dtype=torch.int64)
    doc = torch.tensor([0, 2, 4, 1, 2, 4], dtype=torch.int32)
    tf = torch.tensor([1, 2, 3, 4, 5, 6], dtype=torch.int32)
    keep = np.array([1, 1, 0, 1, 0], np.uint8)
    t, d, f = compact_postings(off, doc, tf, keep)
    assert t.tolist() == [0, 1, 1, 2, 2] and d.tolist() == [0, 1] and f.tolist() == [1, 4]
    t, d, f = compact_postings(off, doc, tf, np.ones(5, bool))
    assert torch.equal(t, off) and torch.equal(d, doc) and torch.equal(f, tf)
    with pytest.raises(ValueError, match="monotone"):
        compact_postings(torch.tensor([0, 3, 2, 5, 6]), doc, tf, keep)
    with pytest.raises(ValueError, match="monotone"):
        compact_postings(torch.tensor([1, 3, 3, 5, 6]), doc, tf, keep)
    with pytest.raises(ValueError, match="outside"):
        compact_postings(off, doc, tf, keep[:4])


def tables_of(docs, V):
    names = [f"t{i}" for i in range(V)]
    postings = {n: [] for n in names}
    for d in sorted(docs):
        for t, c in zip(*np.unique(np.asarray(docs[d], np.int64), return_counts=True)):
            postings[names[t]].append((d, int(c)))
    return postings, {d: len(t) for d, t in docs.items()}


def from_tables(docs, urls_db, chunks, emb, V):
    postings, doc_len = tables_of(docs, V)
    df = np.array([len(postings[f"t{i}"]) for i in range(V)])
    idf = dict(zip([f"t{i}" for i in range(V)], idf_real(len(doc_len), df).tolist()))
    avgdl = np.float32(np.mean(np.array(list(doc_len.values()), np.float64))) if doc_len else 0.0
    return CorpusIndex.from_tables(postings, doc_len, idf, avgdl, chunks=chunks, emb=emb, urls_db=urls_db)


def test_urlsdb_only_documents_and_their_chunks():
    """from_tables indices have documents in urlsDB without a BM25 row (doc_len 0): removing one drops its chunk rows and
    its URL, and total_docs does not move for it."""
    rng = np.random.default_rng(9)
    V = 120
    all_ids = sorted(int(d) for d in rng.choice(5000, 90, replace=False) + 1)
    pending = set(all_ids[::5])                                  # in urlsDB, no bm25_doc_stats row
    toks = {d: list(((rng.zipf(1.3, rng.integers(1, 30)) - 1) % V)) for d in all_ids if d not in pending}
    urls_db = {d: (f"http://h{d % 7}.org/p{d}", f"title {d}", f"text {d}") for d in all_ids}
    chunks = [(c, d) for c, d in enumerate(np.repeat(all_ids, rng.integers(0, 3, len(all_ids))).tolist())]
    emb = {c: rng.standard_normal(DIM).astype(np.float32) for c, _ in chunks}
    ix = from_tables(toks, urls_db, chunks, emb, V)
    gone = sorted(pending)[:6] + [d for d in all_ids if d not in pending][3:9]
    new = remove_documents(ix, np.array(gone))
    assert new.update_counts == dict(removed=12, removed_rows=6, not_found=0)
    assert new.total_docs == ix.total_docs - 6
    rest = [d for d in all_ids if d not in gone]
    want = from_tables({d: toks[d] for d in rest if d in toks}, {d: urls_db[d] for d in rest},
                       [(c, d) for c, d in chunks if d not in gone], emb, V)
    assert_same_tables(new, want)
    assert_same_chunks(new, want)
    assert new.urls == want.urls and new.titles == want.titles and new.texts == want.texts
    assert np.array_equal(new.url_group(), want.url_group())


def chunk_table(rng, doc_ids, first):
    per = rng.integers(0, 4, len(doc_ids))
    own = np.repeat(np.asarray(doc_ids, np.int64), per)
    emb = rng.standard_normal((len(own), DIM)).astype(np.float32)
    return ChunkTable(chunk_ids=np.arange(first, first + len(own), dtype=np.int64), doc_ids=own, seqs=[[1]] * len(own),
                      emb=torch.as_tensor(emb))


def drop_chunks(t, gone):
    k = ~np.isin(t.doc_ids, gone)
    return ChunkTable(chunk_ids=t.chunk_ids[k], doc_ids=t.doc_ids[k], seqs=[s for s, x in zip(t.seqs, k) if x], emb=t.emb[torch.as_tensor(k)])


@pytest.mark.parametrize("pattern", ["scattered", "block"])
def test_remove_chunks(pattern):
    rng = np.random.default_rng(13 + len(pattern))
    b = batch(rng, np.arange(250, dtype=np.int64) * 4 + 2, 200, empty_frac=0.0)
    t0 = chunk_table(rng, b[0], 0)
    ix = attach_chunks(bm25_index_from_token_ids(*b, 200), t0)
    R = removal(rng, np.asarray(ix.doc_ids), pattern)
    before = snapshot(ix)
    new = remove_documents(ix, R)
    for name, arr in before.items():
        assert np.asarray(_np(getattr(ix, name))).tobytes() == arr.tobytes(), name
    want = attach_chunks(bm25_index_from_token_ids(*subset(b, ~np.isin(b[0], R)), 200), drop_chunks(t0, R))
    assert_same_tables(new, want)
    assert_same_chunks(new, want)
    assert new.doc_off.dtype == np.int32
    # an index with chunks and no postings
    bare = CorpusIndex(doc_ids=ix.doc_ids, doc_off=ix.doc_off, chunk_ids=ix.chunk_ids, emb=ix.emb)
    bare.n_docs_global = bare.n_docs
    got = remove_documents(bare, R)
    assert got.term_off is None and np.array_equal(got.doc_ids, want.doc_ids)
    assert_same_chunks(got, want)


def test_url_groups_and_snapshot_roundtrip(tmp_path):
    rng = np.random.default_rng(2)
    b = batch(rng, [10, 15, 20, 30], 50, empty_frac=0.0)
    ix = bm25_index_from_token_ids(*b, 50)
    ix.urls = ["http://a.org/x", "http://c.org/z?page=2", "http://b.org/y", "http://c.org/z"]
    ix.titles, ix.texts = ["A", "C2", "B", "C"], ["a", "c2", "b", "c"]
    g = ix.url_group()
    assert g[1] == g[3]
    new = remove_documents(ix, [30, 20])                         # the ?page=2 URL's base document goes
    assert np.asarray(new.doc_ids).tolist() == [10, 15]
    assert new.urls == ["http://a.org/x", "http://c.org/z?page=2"] and new.titles == ["A", "C2"]
    assert new.url_group().tolist() == [0, 1]                      # it is its own group now
    assert g[1] == g[3]                                           # (the old index keeps its groups)
    new.save_dir(str(tmp_path / "snap"))
    back = CorpusIndex.load_dir(str(tmp_path / "snap"), mmap=False)
    assert_same_tables(back, new)
    assert back.urls == new.urls and np.array_equal(back.url_group(), new.url_group())


@pytest.mark.parametrize("seed", [0, 1])
def test_replace_equals_scratch_build(seed):
    """Replace = remove the old versions, add the new token streams and chunks under the same ids, attach."""
    rng = np.random.default_rng(40 + seed)
    V0, V1 = 180, 220
    ids = np.sort(rng.choice(50_000, 300, replace=False)).astype(np.int64) + 1
    b0 = batch(rng, ids, V0, empty_frac=0.0)
    t0 = chunk_table(rng, ids, 0)
    meta = {int(d): (f"http://s{int(d) % 11}.org/{int(d)}", f"T{int(d)}", f"x{int(d)}") for d in ids}
    ix = attach_chunks(bm25_index_from_token_ids(*b0, V0), t0)
    ix.urls, ix.titles, ix.texts = [[meta[int(d)][j] for d in ix.doc_ids] for j in range(3)]
    R = rng.choice(ids, 40, replace=False)
    rb = batch(rng, np.sort(R), V1, empty_frac=0.0)              # the new versions
    meta2 = {int(d): (f"http://new.org/{int(d)}", f"N{int(d)}", f"y{int(d)}") for d in R}
    removed = remove_documents(ix, R)
    grown = bm25_add_token_ids(removed, *rb, V1, docs_meta=meta2)
    assert grown.update_counts["already_indexed"] == 0 and grown.update_counts["added"] == len(R)
    t1 = chunk_table(rng, np.sort(R), int(np.asarray(ix.chunk_ids).max()) + 1)
    attach_chunks(grown, t1)
    final = concat([subset(b0, ~np.isin(b0[0], R)), rb])
    want = attach_chunks(bm25_index_from_token_ids(*final, V1), drop_chunks(t0, R), t1)
    assert_same_tables(grown, want)
    assert_same_chunks(grown, want)
    m = meta | meta2
    assert grown.urls == [m[int(d)][0] for d in want.doc_ids] and grown.texts == [m[int(d)][2] for d in want.doc_ids]
