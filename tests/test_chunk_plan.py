"""chunk_index.plan_chunks / attach_chunks on the host: documents -> chunk table against a restatement of the reference's
Indexer.index_documents (indexer/indexer.py:95-110; embedder.py:65-87 for the windows), and the row layout of the index
the table is attached to."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
tokenizers = pytest.importorskip("tokenizers")


def _tokenizer(n_words=200):
    """A word-level tokenizer with ModernBERT-style [CLS] ... [SEP] wrapping (written by the test, like
    test_encoder_from_local_directory_and_in_the_retriever's)."""
    from tokenizers import Tokenizer, models, pre_tokenizers, processors
    vocab = {"[UNK]": 0, "[CLS]": 1, "[SEP]": 2}
    vocab.update({f"w{i}": i + 3 for i in range(n_words)})
    tok = Tokenizer(models.WordLevel(vocab, unk_token="[UNK]"))
    tok.pre_tokenizer = pre_tokenizers.Whitespace()
    tok.post_processor = processors.TemplateProcessing(single="[CLS] $A [SEP]", special_tokens=[("[CLS]", 1), ("[SEP]", 2)])
    tok.add_special_tokens(["[CLS]", "[SEP]"])
    return tok


def _ref_windows(tokens, window_size=512, step_size=450):
    """embedder.py:65-87, restated."""
    if len(tokens) <= window_size:
        return [tokens]
    out = []
    for i in range(0, len(tokens) - window_size + 1, step_size):
        out.append(tokens[i:i + window_size])
    last = len(tokens) - window_size
    if last >= 0 and last % step_size != 0:
        out.append(tokens[last:last + window_size])
    return out


def _ref_index_documents(docs, tok, chunk_id):
    """indexer.py:95-110 with the encoder's tokenisation of each window text (sentence-transformers: special tokens on)."""
    rows = []
    for doc_id, title, text in sorted(docs, key=lambda d: d[0]):
        full_text = f"{title or ''} {text or ''}".strip()
        if not full_text:
            continue
        tokens = tok.encode(full_text, add_special_tokens=False).ids
        for w in _ref_windows(tokens):
            window_text = tok.decode(w, skip_special_tokens=True)
            rows.append((chunk_id, doc_id, window_text, tok.encode(window_text).ids))
            chunk_id += 1
    return rows


def _text(rng, n):
    return " ".join(f"w{i}" for i in rng.integers(0, 200, size=n))


def _docs(rng):
    lens = [0, 1, 511, 512, 513, 962, 963, 3000]
    ids = rng.permutation(100)[:len(lens) + 4] + 10          # unsorted doc ids
    docs = []
    for d, n in zip(ids, lens):
        docs.append((int(d), "w199" if n % 2 else None, _text(rng, n) if n else ""))
    docs.append((int(ids[-4]), None, None))                  # empty: no chunk
    docs.append((int(ids[-3]), "", "   "))                   # whitespace only: no chunk
    docs.append((int(ids[-2]), "w5 w6", None))               # title only
    docs.append((int(ids[-1]), None, "w7"))                  # text only
    return docs


@pytest.mark.parametrize("first", [0, 1234])
def test_plan_chunks_text_documents_match_the_reference_loop(first):
    from msretr.chunk_index import plan_chunks
    rng = np.random.default_rng(first + 1)
    tok = _tokenizer()
    docs = _docs(rng)
    want = _ref_index_documents(docs, tok, first)
    got = plan_chunks(docs, tokenizer=tok, first_chunk_id=first)
    assert got.chunk_ids.tolist() == [r[0] for r in want]
    assert got.doc_ids.tolist() == [r[1] for r in want]
    assert got.texts == [r[2] for r in want]
    assert got.seqs == [r[3] for r in want]
    assert all(s[0] == 1 and s[-1] == 2 and len(s) <= 514 for s in got.seqs)
    per_doc = {}
    for d in got.doc_ids.tolist():
        per_doc[d] = per_doc.get(d, 0) + 1
    # windows per document: <= 512 tokens -> 1; 513 -> 2 (0, 1); 962 -> 2 (0, 450); 963 -> 3 (0, 450, 451);
    # 3000 -> 7 (0, 450, ..., 2250, 2488).  The one-word title adds a token to the documents of odd length.
    n_tokens = {d: len(tok.encode(f"{t or ''} {x or ''}".strip(), add_special_tokens=False).ids)
                for d, t, x in docs if f"{t or ''} {x or ''}".strip()}
    expect = {1: 1, 512: 1, 513: 2, 514: 2, 962: 2, 963: 3, 964: 3, 3000: 7, 3001: 7, 2: 1}
    for d, n in n_tokens.items():
        if n in expect:
            assert per_doc[d] == expect[n], (d, n, per_doc[d])
    assert got.next_chunk_id == first + len(want)


def test_plan_chunks_token_id_documents():
    from msretr.chunk_index import plan_chunks
    rng = np.random.default_rng(5)
    lens = [3000, 0, 1, 511, 512, 513, 962, 963]
    ids = [50, 7, 9, 3, 11, 2, 40, 8]
    docs = [(d, rng.integers(0, 1000, size=n).tolist()) for d, n in zip(ids, lens)]
    got = plan_chunks(docs, cls_id=50281, sep_id=50282, first_chunk_id=10)
    want_seqs, want_doc = [], []
    for d, t in sorted(docs):
        if not t:
            continue
        for w in _ref_windows(t):
            want_seqs.append([50281] + w + [50282])
            want_doc.append(d)
    assert got.seqs == want_seqs and got.doc_ids.tolist() == want_doc and got.texts is None
    assert got.chunk_ids.tolist() == list(range(10, 10 + len(want_seqs)))
    bare = plan_chunks(docs)
    assert bare.seqs == [s[1:-1] for s in want_seqs]
    with pytest.raises(ValueError):
        plan_chunks([(1, [1, 2]), (1, [3])])                  # duplicate doc_id
    with pytest.raises(ValueError):
        plan_chunks([(1, "title", "text")])                   # text without a tokenizer


def _fake_table(plan, seed):
    """Embeddings that name their chunk: row i = chunk_id in column 0, random elsewhere."""
    g = torch.Generator().manual_seed(seed)
    emb = torch.randn(len(plan), 768, generator=g)
    emb[:, 0] = torch.as_tensor(plan.chunk_ids, dtype=torch.float32)
    plan.emb = emb
    return plan


def test_attach_chunks_row_order_doc_off_and_append():
    from msretr.chunk_index import attach_chunks, plan_chunks
    from msretr.index_build import bm25_index_from_token_ids
    rng = np.random.default_rng(11)
    lens = [700, 5, 1200, 0, 513, 40]
    ids = [31, 4, 17, 22, 9, 50]
    toks = [rng.integers(0, 300, size=n).tolist() for n in lens]
    off = np.concatenate([[0], np.cumsum(lens)])
    ix = bm25_index_from_token_ids(ids, off, np.concatenate(toks).astype(np.int32), 300, device="cpu")
    docs = list(zip(ids, toks))
    first = _fake_table(plan_chunks(docs[:3], cls_id=1, sep_id=2), 0)
    ix = attach_chunks(ix, first)

    def check(ix, tables):
        doc_ids = np.asarray(ix.doc_ids)
        rank = {int(d): i for i, d in enumerate(doc_ids)}
        rows = sorted((rank[int(d)], int(c)) for t in tables for c, d in zip(t.chunk_ids, t.doc_ids))
        assert np.asarray(ix.chunk_ids).tolist() == [c for _, c in rows]
        cnt = np.bincount([r for r, _ in rows], minlength=len(doc_ids))
        assert np.asarray(ix.doc_off).tolist() == np.concatenate([[0], np.cumsum(cnt)]).tolist()
        assert ix.n_chunks == len(rows)
        assert ix.emb[:, 0].tolist() == [float(c) for _, c in rows]       # every row travelled with its chunk
        by_id = {int(c): e for t in tables for c, e in zip(t.chunk_ids, t.emb)}
        for i, (_, c) in enumerate(rows):
            assert torch.equal(ix.emb[i], by_id[c])

    check(ix, [first])
    # "unindexed documents only": a later call numbers its chunks on from the first table's MAX(chunk_id) + 1
    second = _fake_table(plan_chunks(docs[3:], cls_id=1, sep_id=2, first_chunk_id=first.next_chunk_id), 1)
    assert int(second.chunk_ids[0]) == int(first.chunk_ids[-1]) + 1
    ix = attach_chunks(ix, second)
    check(ix, [first, second])
    with pytest.raises(ValueError):
        attach_chunks(ix, second)                             # the same chunk ids again
    stray = _fake_table(plan_chunks([(999, [1, 2, 3])], first_chunk_id=10_000), 2)
    with pytest.raises(ValueError):
        attach_chunks(ix, stray)                              # a document the index does not have
