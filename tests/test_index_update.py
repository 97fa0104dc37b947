"""Adding documents to a built BM25 index (index_build.bm25_add_token_ids, CPU device): the updated tables must equal a
from-scratch build of the union bit for bit, as the reference's incremental BM25.build_index recomputes avg_doc_length and
the idf of every term (indexer/bm25_indexer.py:252-369, :130-147)."""
import numpy as np
import pytest
import torch

from msretr.chunk_index import ChunkTable, attach_chunks
from msretr.index import DIM, CorpusIndex, _np
from msretr.index_build import bm25_add_token_ids, bm25_index_from_token_ids, idf_real, merge_postings

TABLES = ("doc_ids", "doc_len", "term_off", "post_doc", "post_tf", "idf")


def batch(rng, ids, n_terms, empty_frac=0.15, max_len=40):
    """Token-id streams of documents `ids` (some without tokens), Zipf-like term ids below n_terms."""
    lens = rng.integers(1, max_len, len(ids))
    lens[rng.random(len(ids)) < empty_frac] = 0
    off = np.zeros(len(ids) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    tok = ((rng.zipf(1.3, int(off[-1])) - 1) % n_terms).astype(np.int32)
    return np.asarray(ids, np.int64), off, tok


def concat(batches):
    ids = np.concatenate([b[0] for b in batches])
    off = np.concatenate([[0], np.cumsum(np.concatenate([np.diff(b[1]) for b in batches]))]).astype(np.int64)
    tok = np.concatenate([b[2] for b in batches])
    return ids, off, tok


def subset(b, keep):
    """The documents of batch b where keep is True, with their tokens."""
    ids, off, tok = b
    idx = np.nonzero(keep)[0]
    lens = np.diff(off)[idx]
    parts = [tok[off[i]:off[i + 1]] for i in idx]
    return ids[idx], np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), np.concatenate(parts + [np.zeros(0, np.int32)])


def assert_same_tables(got, want):
    for name in TABLES:
        g, w = np.asarray(_np(getattr(got, name))), np.asarray(_np(getattr(want, name)))
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), name
    assert np.float32(got.avgdl).tobytes() == np.float32(want.avgdl).tobytes()
    assert got.total_docs == want.total_docs and got.n_docs_global == got.n_docs


def snapshot(ix):
    return {n: np.asarray(_np(getattr(ix, n))).copy() for n in TABLES}


def split_ids(rng, pattern, n, parts):
    """n distinct doc ids split into `parts` batches: appended (every batch above the previous ones) or interleaved."""
    ids = np.sort(rng.choice(20 * n, n, replace=False)).astype(np.int64) + 7
    if pattern == "appended":
        cuts = np.sort(rng.choice(np.arange(1, n), parts - 1, replace=False))
        return np.split(ids, cuts)
    which = rng.integers(0, parts, n)
    which[:parts] = np.arange(parts)
    return [rng.permutation(ids[which == p]) for p in range(parts)]


@pytest.mark.parametrize("pattern", ["appended", "interleaved", "reindexed"])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_update_equals_scratch_build(pattern, seed):
    rng = np.random.default_rng(100 * seed + len(pattern))
    parts = 2 + seed                                   # base + 1..3 update batches
    groups = split_ids(rng, "appended" if pattern == "appended" else "interleaved", 300, parts)
    vocab = np.sort(rng.integers(20, 400, parts))      # the vocabulary grows batch after batch
    batches = [batch(rng, g, int(v)) for g, v in zip(groups, vocab)]
    ix = bm25_index_from_token_ids(*batches[0], int(vocab[0]))
    applied = [batches[0]]
    for k in range(1, parts):
        b = batches[k]
        if pattern == "reindexed":
            # documents the index already has (with other tokens: skipped, not re-processed) and documents without tokens
            old = concat(applied)
            again = rng.choice(len(old[0]), 20, replace=False)
            extra = batch(rng, old[0][again], int(vocab[k]), empty_frac=0.3)
            fresh_empty = (np.arange(5, dtype=np.int64) + 10_000_000 * (k + 1), np.zeros(6, np.int64), np.zeros(0, np.int32))
            b = concat([b, extra, fresh_empty])
            perm = rng.permutation(len(b[0]))
            lens = np.diff(b[1])[perm]
            off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
            tok = np.concatenate([b[2][b[1][i]:b[1][i + 1]] for i in perm]) if len(perm) else b[2]
            b = (b[0][perm], off, tok)
        before = snapshot(ix)
        new = bm25_add_token_ids(ix, *b, int(vocab[k]))
        for name, arr in before.items():                 # the old index is left as it was
            assert np.asarray(_np(getattr(ix, name))).tobytes() == arr.tobytes()
        if pattern == "reindexed":
            known = np.isin(b[0], concat(applied)[0][np.diff(concat(applied)[1]) > 0])
            assert new.update_counts["already_indexed"] == int(known.sum())
            b = subset(b, ~known)
            # a tokenless document of an earlier batch that now has tokens is the batch's (once) in the union
            applied = [subset(a, ~(np.isin(a[0], b[0]) & (np.diff(a[1]) == 0))) for a in applied]
        applied.append(b)
        ix = new
        assert_same_tables(ix, bm25_index_from_token_ids(*concat(applied), int(vocab[k])))


def test_only_touched_idf_refresh_is_caught():
    """Negative control: refreshing the idf of the batch's terms only (leaving the rest at the old N) differs from the
    reference, which recomputes every row of bm25_term_stats."""
    rng = np.random.default_rng(5)
    base, upd = batch(rng, np.arange(200) * 3, 300), batch(rng, np.arange(200, 260) * 3, 300)
    ix = bm25_index_from_token_ids(*base, 300)
    new = bm25_add_token_ids(ix, *upd, 300)
    want = bm25_index_from_token_ids(*concat([base, upd]), 300)
    assert_same_tables(new, want)
    touched = np.zeros(300, bool)
    touched[np.unique(upd[2])] = True
    df = np.diff(np.asarray(_np(new.term_off)))
    partial = np.asarray(_np(ix.idf)).copy()
    partial[touched] = idf_real(new.total_docs, df)[touched]
    assert partial.tobytes() != np.asarray(_np(want.idf)).tobytes()


def tables_of(docs, V):
    """Reference-style tables (CorpusIndex.from_tables input) of {doc_id: token ids}: postings by term name, doc lengths."""
    names = [f"t{i}" for i in range(V)]
    postings = {n: [] for n in names}
    for d in sorted(docs):
        toks = docs[d]
        for t, c in zip(*np.unique(np.asarray(toks, np.int64), return_counts=True)):
            postings[names[t]].append((d, int(c)))
    return postings, {d: len(t) for d, t in docs.items()}


def test_duckdb_shaped_update():
    """The base comes from reference tables whose urlsDB has documents without a bm25_doc_stats row: the update gives them
    their rows (keeping their dense indices) and adds new documents; the result equals from_tables over the full tables."""
    rng = np.random.default_rng(9)
    V0, V1 = 150, 180
    toks = {int(d): list(((rng.zipf(1.3, rng.integers(1, 30)) - 1) % V0)) for d in rng.choice(5000, 120, replace=False) + 1}
    all_ids = sorted(toks)
    pending = set(all_ids[::4])                                  # in urlsDB, not yet BM25-indexed
    fresh = {int(d): list(((rng.zipf(1.3, rng.integers(1, 30)) - 1) % V1)) for d in rng.choice(5000, 30, replace=False) + 6000}
    urls_db = {d: (f"http://h{d % 7}.org/p{d}", f"title {d}", f"text {d}") for d in all_ids + sorted(fresh)}

    def build(docs, url_ids, V):
        postings, doc_len = tables_of(docs, V)
        df = np.array([len(postings[f"t{i}"]) for i in range(V)])
        idf = dict(zip([f"t{i}" for i in range(V)], idf_real(len(doc_len), df).tolist()))
        avgdl = np.float32(np.mean(np.array(list(doc_len.values()), np.float64)))
        return CorpusIndex.from_tables(postings, doc_len, idf, avgdl, urls_db={d: urls_db[d] for d in url_ids})

    base = build({d: toks[d] for d in all_ids if d not in pending}, all_ids, V0)
    batch_docs = {d: toks[d] for d in pending} | fresh
    ids = np.array(sorted(batch_docs), np.int64)
    off = np.concatenate([[0], np.cumsum([len(batch_docs[d]) for d in ids])]).astype(np.int64)
    tok = np.concatenate([np.asarray(batch_docs[d], np.int32) for d in ids])
    new = bm25_add_token_ids(base, ids, off, tok, V1, vocab={f"t{i}": i for i in range(V1)},
                             docs_meta={d: urls_db[d] for d in fresh})
    want = build(toks | fresh, all_ids + sorted(fresh), V1)
    assert_same_tables(new, want)
    pos = {int(d): i for i, d in enumerate(np.asarray(base.doc_ids))}
    new_pos = {int(d): i for i, d in enumerate(np.asarray(new.doc_ids))}
    assert all(new_pos[d] == pos[d] for d in all_ids)           # (the new ids are all above the old ones)
    assert new.urls == want.urls and new.titles == want.titles and new.texts == want.texts
    assert np.array_equal(new.url_group(), want.url_group())
    assert new.update_counts == dict(added=len(batch_docs), already_indexed=0, no_tokens=0)
    assert new.vocab == want.vocab


def test_pending_documents_keep_dense_index():
    rng = np.random.default_rng(4)
    postings, doc_len = tables_of({1: [0, 1], 5: [1, 2, 2]}, 4)
    idf = {f"t{i}": 0.0 for i in range(4)}
    base = CorpusIndex.from_tables(postings, doc_len, idf, 2.5, urls_db={i: (f"u{i}", "t", "x") for i in (1, 3, 5)})
    b = batch(rng, [3], 4, empty_frac=0.0)
    new = bm25_add_token_ids(base, *b, 4)
    assert np.asarray(new.doc_ids).tolist() == [1, 3, 5]
    assert np.asarray(_np(new.doc_len)).tolist() == [2, len(b[2]), 3]
    assert new.total_docs == 3


def chunk_table(rng, doc_ids, first):
    per = rng.integers(0, 4, len(doc_ids))
    own = np.repeat(np.asarray(doc_ids, np.int64), per)
    emb = rng.standard_normal((len(own), DIM)).astype(np.float32)
    return ChunkTable(chunk_ids=np.arange(first, first + len(own), dtype=np.int64), doc_ids=own, seqs=[[1]] * len(own),
                      emb=torch.as_tensor(emb))


@pytest.mark.parametrize("pattern", ["appended", "interleaved"])
def test_update_then_attach_chunks(pattern):
    rng = np.random.default_rng(11)
    g0, g1 = split_ids(rng, pattern, 200, 2)
    b0, b1 = batch(rng, g0, 120, empty_frac=0.0), batch(rng, g1, 160, empty_frac=0.0)
    t0 = chunk_table(rng, np.sort(g0), 0)
    t1 = chunk_table(rng, np.sort(g1), t0.next_chunk_id or 0)
    ix = attach_chunks(bm25_index_from_token_ids(*b0, 120), t0)
    emb_before = ix.emb.clone()
    new = bm25_add_token_ids(ix, *b1, 160)
    assert new.n_chunks == ix.n_chunks and np.array_equal(np.diff(np.asarray(new.doc_off))[np.isin(new.doc_ids, g1)], 0 * g1)
    attach_chunks(new, t1)
    want = attach_chunks(bm25_index_from_token_ids(*concat([b0, b1]), 160), t0, t1)
    assert_same_tables(new, want)
    assert np.array_equal(np.asarray(new.doc_off), np.asarray(want.doc_off))
    assert np.array_equal(np.asarray(new.chunk_ids), np.asarray(want.chunk_ids))
    assert torch.equal(new.emb, want.emb)
    assert torch.equal(ix.emb, emb_before) and ix.n_chunks == len(t0)


def test_url_groups_and_snapshot_roundtrip(tmp_path):
    rng = np.random.default_rng(2)
    base_b = batch(rng, [10, 20, 30], 50, empty_frac=0.0)
    ix = bm25_index_from_token_ids(*base_b, 50)
    ix.urls = ["http://a.org/x", "http://b.org/y?id=1", "http://c.org/z"]
    ix.titles = ["A", "B", "C"]
    ix.texts = ["a", "b", "c"]
    assert ix.url_group().tolist() == [0, 1, 2]               # (cached on the old index: must not leak into the new one)
    upd = batch(rng, [15, 40], 60, empty_frac=0.0)
    new = bm25_add_token_ids(ix, *upd, 60, docs_meta={15: ("http://c.org/z?page=2", "C2", "c2"), 40: ("http://d.org/", "D", "d")})
    assert np.asarray(new.doc_ids).tolist() == [10, 15, 20, 30, 40]
    assert new.urls[1] == "http://c.org/z?page=2" and new.titles[4] == "D"
    g = new.url_group()
    assert g[1] == g[3] and len(set(g.tolist())) == 4              # the ?page=2 URL joins the old document's group
    new.save_dir(str(tmp_path / "snap"))
    back = CorpusIndex.load_dir(str(tmp_path / "snap"), mmap=False)
    assert_same_tables(back, new)
    assert back.urls == new.urls and np.array_equal(back.url_group(), g)


def test_refusals():
    rng = np.random.default_rng(3)
    b0 = batch(rng, np.arange(40) * 2, 30, empty_frac=0.0)
    ix = bm25_index_from_token_ids(*b0, 30)
    upd = batch(rng, np.arange(40, 50) * 2, 30, empty_frac=0.0)
    with pytest.raises(ValueError, match="shard"):
        bm25_add_token_ids(ix.shard(1, 2), *upd, 30)
    with pytest.raises(ValueError, match="shard"):
        bm25_add_token_ids(ix.shard(0, 2), *upd, 30)
    bad = (upd[0], upd[1], upd[2].copy())
    bad[2][0] = 31
    with pytest.raises(ValueError, match="n_terms"):
        bm25_add_token_ids(ix, *bad, 31)
    with pytest.raises(ValueError, match="shrink"):
        bm25_add_token_ids(ix, *upd, 29)
    dup = (np.array([500, 500], np.int64), np.array([0, 1, 2], np.int64), np.array([1, 2], np.int32))
    with pytest.raises(ValueError, match="duplicate"):
        bm25_add_token_ids(ix, *dup, 30)


def test_merge_postings_cpu_clash_and_maps():
    off = torch.tensor([0, 2], dtype=torch.int64)
    a = (off, torch.tensor([0, 1], dtype=torch.int32), torch.tensor([1, 1], dtype=torch.int32))
    b = (torch.tensor([0, 1], dtype=torch.int64), torch.tensor([0], dtype=torch.int32), torch.tensor([5], dtype=torch.int32))
    t, d, f = merge_postings(a[0], a[1], a[2], np.array([0, 2], np.int32), *b, np.array([1], np.int32), 1, 3)
    assert t.tolist() == [0, 3] and d.tolist() == [0, 1, 2] and f.tolist() == [1, 5, 1]
    with pytest.raises(ValueError, match="both sides"):
        merge_postings(*a, np.array([0, 2], np.int32), *b, np.array([2], np.int32), 1, 3)
    with pytest.raises(ValueError, match="strictly increasing"):
        merge_postings(*a, np.array([2, 0], np.int32), *b, np.array([1], np.int32), 1, 3)
