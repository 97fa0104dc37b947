"""BM25 index build from tokenised documents (host-side, offline like the reference's).

Produces the same tables as BM25.build_index (indexer/bm25_indexer.py:16-54, 203-250, 346-369, 130-147) from
already-tokenised documents -- the spaCy lemmatiser stays external:
  * a document with no tokens gets no bm25_doc_stats row (:224, :45-46)
  * doc_length = number of tokens, freq = occurrences of the term in the document (:47-53)
  * total_docs = COUNT(*) of bm25_doc_stats, avg_doc_length = AVG(doc_length), both stored REAL (float32)
  * idf = LOG((N - df + 0.5) / (df + 0.5)) evaluated by DuckDB (LOG = log10) and stored REAL
The result is a CorpusIndex in the engine's layout (CSR by term, documents ascending inside a term).
"""
from collections import Counter

import math

import numpy as np

from .index import CorpusIndex
from .text import CITY


def normalise_document_text(title, text):
    """What the reference feeds to the tokeniser: title + text, lower-cased, city spellings unified, capped at
    1 M characters (bm25_indexer.py:30-32)."""
    s = f"{title or ''} {text or ''}".lower().replace("tuebingen", CITY).replace("tubingen", CITY)
    return s[:1_000_000]


def idf_real(total_docs, doc_freq):
    """idf_score of every term at once: LOG((N - df + 0.5) / (df + 0.5)) (bm25_indexer.py:138; DuckDB's LOG is log10) in
    float64, stored REAL (float32); N itself round-trips through a REAL column (:361-364, :133).  doc_freq: integer array."""
    n_real = float(np.float32(total_docs))
    df = np.asarray(doc_freq, np.float64)
    ratio = (n_real - df + 0.5) / (df + 0.5)
    # the logarithm goes through libm's log10 (what DuckDB's LOG and the reference-executed fixture resolve to): numpy's
    # vectorised log10 differs from it in the last float64 ulp on ~1.6 % of inputs, which could flip a float32 rounding.
    # Evaluated once per DISTINCT document frequency (a Zipfian vocabulary has few of them).
    uniq, inv = np.unique(ratio, return_inverse=True)
    logs = np.fromiter((math.log10(x) for x in uniq.tolist()), np.float64, len(uniq))
    return logs[inv].reshape(ratio.shape).astype(np.float32)


def bm25_index_from_tokens(doc_ids, token_lists, k1=1.2, b=0.75, keep_tokens=False):
    """doc_ids: iterable of int; token_lists: one list of term strings per document.  keep_tokens=True: the kept documents'
    streams stay on the index as its forward index (tok_off / tok_ids, phrase search)."""
    rows = sorted(((int(d), toks) for d, toks in zip(doc_ids, token_lists) if toks), key=lambda r: r[0])
    ids = np.array([d for d, _ in rows], np.int64)
    if len(set(ids.tolist())) != len(ids):
        raise ValueError("duplicate doc_id")
    vocab, postings = {}, []                       # postings[t] = [(doc index, tf)] in ascending doc order
    doc_len = np.zeros(len(rows), np.int32)
    for i, (_, toks) in enumerate(rows):
        doc_len[i] = len(toks)
        for term, tf in Counter(toks).items():
            t = vocab.setdefault(term, len(vocab))
            if t == len(postings):
                postings.append([])
            postings[t].append((i, tf))
    V, N = len(vocab), len(rows)
    term_off = np.zeros(V + 1, np.int64)
    term_off[1:] = np.cumsum([len(p) for p in postings])
    post_doc = np.fromiter((d for p in postings for d, _ in p), np.int32, count=int(term_off[-1]))
    post_tf = np.fromiter((tf for p in postings for _, tf in p), np.int32, count=int(term_off[-1]))
    idf = idf_real(N, np.diff(term_off))
    avgdl = float(np.float32(doc_len.astype(np.float64).mean())) if N else 0.0
    ix = CorpusIndex(doc_ids=ids, doc_len=doc_len, term_off=term_off, post_doc=post_doc, post_tf=post_tf, idf=idf,
                     avgdl=avgdl, total_docs=N, k1=k1, b=b, vocab=vocab)
    ix.n_docs_global = N
    if keep_tokens:
        ix.tok_off = np.zeros(N + 1, np.int64)
        ix.tok_off[1:] = np.cumsum(doc_len)
        ix.tok_ids = np.fromiter((vocab[t] for _, toks in rows for t in toks), np.int32, count=int(ix.tok_off[-1]))
    return ix


def _gather_streams(tok_off, tok_ids, docs):
    """The streams of documents `docs` (indices into tok_off, any order) back to back -> (offsets int64 [len(docs) + 1] on the
    host, ids: one gather of tok_ids, which may be a torch tensor on any device or a numpy array)."""
    import torch
    off = np.asarray(tok_off.cpu() if torch.is_tensor(tok_off) else tok_off, np.int64)
    docs = np.asarray(docs, np.int64)
    lens = off[docs + 1] - off[docs]
    k_off = np.zeros(len(docs) + 1, np.int64)
    k_off[1:] = np.cumsum(lens)
    src = np.repeat(off[docs] - k_off[:-1], lens) + np.arange(k_off[-1])
    if torch.is_tensor(tok_ids):
        return k_off, tok_ids[torch.as_tensor(src, device=tok_ids.device)].contiguous()
    return k_off, np.asarray(tok_ids)[src]


def bm25_index_from_token_ids(doc_ids, tok_off, tok_ids, n_terms, device="cpu", k1=1.2, b=0.75, vocab=None, keep_tokens=False):
    """The same tables from token-id streams, built on `device` (the build given pre-tokenised
    documents, at corpus scale: one radix sort of (term, document) keys + run lengths instead of Python dicts).

    doc_ids int64 [N]; tok_off int64 [N+1]; tok_ids int32 [T] with document i's tokens at tok_off[i]:tok_off[i+1], term
    ids in [0, n_terms).  Documents without tokens get no row (bm25_indexer.py:224); documents are numbered by
    ascending doc_id; inside a term the postings ascend by document.  On a GPU device the tables come from the hand-written
    kernels of csrc/msr_build.hip (per-document sort + run lengths, stable radix sort by term, boundary-based doc_freq,
    three-kernel scans; msr_build_postings); on the CPU device torch's sort / unique_consecutive / bincount restate the same
    build (host-side reference for the tests).  idf is evaluated on the host with the same float64 log10 -> float32
    rounding as bm25_index_from_tokens so that all builders agree bit for bit.

    keep_tokens=True: the streams of the kept documents (those with tokens, ascending doc_id) stay on the index as its forward
    index -- tok_off int64 [N+1], tok_ids int32 [T] on `device`, never the caller's own tensor -- lengths and their cumulative
    sum on the host (numpy, N values), the ids in one torch gather on `device`.
    What phrase search reads (DeviceEngine.phrase_sets); off by default."""
    import torch
    dev = torch.device(device)
    if dev.type == "cuda":
        return _bm25_index_from_token_ids_hip(doc_ids, tok_off, tok_ids, n_terms, dev, k1, b, vocab, keep_tokens)
    ids = torch.as_tensor(np.asarray(doc_ids, np.int64))
    off = torch.as_tensor(np.asarray(tok_off, np.int64)).to(dev)
    tok = (tok_ids if torch.is_tensor(tok_ids) else torch.as_tensor(np.asarray(tok_ids, np.int32))).to(dev)
    if len(set(ids.tolist())) != len(ids):
        raise ValueError("duplicate doc_id")
    lens = (off[1:] - off[:-1])
    if tok.numel() and (int(tok.min()) < 0 or int(tok.max()) >= n_terms):
        raise ValueError("token id outside [0, n_terms)")
    order = torch.argsort(ids).to(dev)                                      # ascending doc_id
    keep = order[lens[order] > 0]                                           # documents with tokens, in id order
    N = int(keep.numel())
    rank = torch.full((len(ids),), -1, dtype=torch.int64, device=dev)
    rank[keep] = torch.arange(N, device=dev)
    tok_doc = torch.repeat_interleave(rank, lens)                           # dense document index of every token
    key = tok.to(torch.int64) * max(N, 1) + tok_doc                         # (term, document): tokens of dropped docs have none
    key = torch.sort(key).values
    uniq, tf = torch.unique_consecutive(key, return_counts=True)
    p_term, p_doc = uniq // max(N, 1), uniq % max(N, 1)
    df = torch.bincount(p_term, minlength=n_terms)
    term_off = torch.zeros(n_terms + 1, dtype=torch.int64, device=dev)
    term_off[1:] = torch.cumsum(df, 0)
    doc_len = lens[keep].to(torch.int32)
    idf = idf_real(N, df.cpu().numpy())
    avgdl = float(np.float32(doc_len.to(torch.float64).mean().item())) if N else 0.0
    ix = CorpusIndex(doc_ids=ids[keep.cpu()].numpy(), doc_len=doc_len, term_off=term_off, post_doc=p_doc.to(torch.int32),
                     post_tf=tf.to(torch.int32), idf=torch.as_tensor(idf).to(dev), avgdl=avgdl, total_docs=N, k1=k1, b=b,
                     vocab=vocab)
    ix.n_docs_global = N
    if keep_tokens:
        k_off, k_tok = _gather_streams(off, tok, keep.cpu().numpy())
        ix.tok_off, ix.tok_ids = torch.as_tensor(k_off).to(dev), k_tok.to(torch.int32)
    return ix


def _bm25_index_from_token_ids_hip(doc_ids, tok_off, tok_ids, n_terms, dev, k1, b, vocab, keep_tokens=False):
    """bm25_index_from_token_ids on the GPU through the C ABI (msr_build_postings); no fallback."""
    import ctypes as C

    import torch

    from . import _abi
    lib = _abi.load()
    ids = np.asarray(doc_ids, np.int64)
    if len(set(ids.tolist())) != len(ids):
        raise ValueError("duplicate doc_id")
    off = np.asarray(tok_off.cpu() if torch.is_tensor(tok_off) else tok_off, np.int64)
    tok = (tok_ids if torch.is_tensor(tok_ids) else torch.as_tensor(np.asarray(tok_ids, np.int32))).to(dev, torch.int32).contiguous()
    if tok.numel() and (int(tok.min()) < 0 or int(tok.max()) >= n_terms):
        raise ValueError("token id outside [0, n_terms)")
    lens = np.diff(off)
    order = np.argsort(ids, kind="stable")
    keep = order[lens[order] > 0]                                           # documents with tokens, ascending doc_id
    N = len(keep)
    # the kernels want the kept documents' tokens back to back in that order: one gather of token ranges (skipped when the
    # input already is in that shape)
    if N == len(ids) and np.array_equal(keep, np.arange(N)):
        k_off, k_tok = off, tok
    else:
        k_off = np.zeros(N + 1, np.int64); k_off[1:] = np.cumsum(lens[keep])
        src = torch.as_tensor(np.repeat(off[keep] - k_off[:-1], lens[keep]) + np.arange(k_off[-1]), device=dev)
        k_tok = tok[src].contiguous()
    d_off = torch.as_tensor(k_off).to(dev)
    term_off = torch.empty(n_terms + 1, dtype=torch.int64, device=dev)
    n_post = C.c_int64(0)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else C.c_void_p(0)
    with torch.cuda.device(dev):
        _abi.check(None, lib.msr_build_postings(ptr(d_off), ptr(k_tok), N, int(n_terms), ptr(term_off), C.c_void_p(0), C.c_void_p(0), 0,
                                                C.byref(n_post), stream))
        P = int(n_post.value)
        post_doc = torch.empty(max(P, 1), dtype=torch.int32, device=dev)
        post_tf = torch.empty(max(P, 1), dtype=torch.int32, device=dev)
        _abi.check(None, lib.msr_build_postings(ptr(d_off), ptr(k_tok), N, int(n_terms), ptr(term_off), ptr(post_doc), ptr(post_tf), max(P, 1),
                                                C.byref(n_post), stream))
    idf = idf_real(N, np.diff(term_off.cpu().numpy()))
    doc_len = torch.as_tensor(lens[keep].astype(np.int32)).to(dev)
    avgdl = float(np.float32(lens[keep].astype(np.float64).mean())) if N else 0.0
    ix = CorpusIndex(doc_ids=ids[keep], doc_len=doc_len, term_off=term_off, post_doc=post_doc[:P], post_tf=post_tf[:P],
                     idf=torch.as_tensor(idf).to(dev), avgdl=avgdl, total_docs=N, k1=k1, b=b, vocab=vocab)
    ix.n_docs_global = N
    if keep_tokens:                                          # the builder's own input; a copy where that still is the caller's tensor
        ix.tok_off, ix.tok_ids = d_off, (k_tok.clone() if k_tok is tok_ids else k_tok)
    return ix


# ---------------------------------------------------------------------------------------------------------------- updates
def merge_postings(a_term_off, a_doc, a_tf, a_map, b_term_off, b_doc, b_tf, b_map, n_terms, n_docs, device="cpu", a_docs=None):
    """Two CSR-by-term posting tables -> one (msr_merge_postings on a GPU device; a torch / numpy restatement on the CPU).
    Side A (a built index) and side B (new documents) each: term_off [terms + 1], doc / tf [postings] with documents strictly
    ascending inside a term, and a strictly increasing map of its dense document indices into [0, n_docs) (a_map None =
    identity over a_docs documents, default n_docs).  Returns (term_off int64 [n_terms + 1], post_doc int32, post_tf int32)
    tensors on `device`: inside a term the two segments merged by mapped document, post_doc = the mapped index.  The same merged document in one term on both sides
    raises (ValueError on the CPU, MsrError on the GPU): postings are never merged silently."""
    import torch
    from .index import _np
    dev = torch.device(device)
    if dev.type == "cuda":
        return _merge_postings_hip(a_term_off, a_doc, a_tf, a_map, b_term_off, b_doc, b_tf, b_map, n_terms, n_docs, dev, a_docs)
    a_off, b_off = np.asarray(_np(a_term_off), np.int64), np.asarray(_np(b_term_off), np.int64)
    a_terms, b_terms = len(a_off) - 1, len(b_off) - 1
    if n_terms < max(a_terms, b_terms):
        raise ValueError("n_terms is smaller than a side's vocabulary")
    a_doc, b_doc = np.asarray(_np(a_doc), np.int64)[:a_off[-1]], np.asarray(_np(b_doc), np.int64)[:b_off[-1]]
    keys = []
    for m, d in ((a_map, a_doc), (b_map, b_doc)):
        if m is None:
            if len(d) and (d.min() < 0 or d.max() >= (n_docs if a_docs is None else a_docs)):
                raise ValueError("a posting's document index is outside its side's documents")
            keys.append(d)
            continue
        m = np.asarray(_np(m), np.int64)
        if len(m) and (m.min() < 0 or m.max() >= n_docs or np.any(np.diff(m) <= 0)):
            raise ValueError("a document map is out of [0, n_docs) or not strictly increasing")
        keys.append(m[d])
    a_term = np.repeat(np.arange(a_terms, dtype=np.int64), np.diff(a_off))
    b_term = np.repeat(np.arange(b_terms, dtype=np.int64), np.diff(b_off))
    key = np.concatenate([a_term * max(n_docs, 1) + keys[0], b_term * max(n_docs, 1) + keys[1]])
    order = np.argsort(key, kind="stable")
    sk = key[order]
    if np.any(sk[1:] == sk[:-1]):
        raise ValueError("the same merged document has postings of one term on both sides")
    t = np.arange(n_terms + 1)
    term_off = a_off[np.minimum(t, a_terms)] + b_off[np.minimum(t, b_terms)]
    post_doc = np.concatenate(keys)[order].astype(np.int32)
    post_tf = np.concatenate([np.asarray(_np(a_tf), np.int32)[:a_off[-1]], np.asarray(_np(b_tf), np.int32)[:b_off[-1]]])[order]
    return torch.as_tensor(term_off), torch.as_tensor(post_doc), torch.as_tensor(post_tf)


def _merge_postings_hip(a_term_off, a_doc, a_tf, a_map, b_term_off, b_doc, b_tf, b_map, n_terms, n_docs, dev, a_docs):
    """merge_postings through the C ABI (msr_merge_postings); no fallback."""
    import ctypes as C

    import torch

    from . import _abi
    lib = _abi.load()

    def on_dev(x, dtype):
        if x is None:
            return None
        t = x if torch.is_tensor(x) else torch.as_tensor(np.ascontiguousarray(x))
        return t.to(dev, dtype).contiguous()
    a_off, b_off = on_dev(a_term_off, torch.int64), on_dev(b_term_off, torch.int64)
    a_doc, a_tf, b_doc, b_tf = (on_dev(x, torch.int32) for x in (a_doc, a_tf, b_doc, b_tf))
    a_map, b_map = on_dev(a_map, torch.int32), on_dev(b_map, torch.int32)
    a_docs = int(a_map.numel()) if a_map is not None else int(n_docs if a_docs is None else a_docs)
    b_docs = int(b_map.numel()) if b_map is not None else 0
    P = int(a_off[-1].item()) + int(b_off[-1].item())
    term_off = torch.empty(int(n_terms) + 1, dtype=torch.int64, device=dev)
    post_doc = torch.empty(max(P, 1), dtype=torch.int32, device=dev)
    post_tf = torch.empty(max(P, 1), dtype=torch.int32, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else C.c_void_p(0)
    with torch.cuda.device(dev):
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _abi.check(None, lib.msr_merge_postings(ptr(a_off), int(a_off.numel()) - 1, ptr(a_doc), ptr(a_tf), ptr(a_map), a_docs,
                                                ptr(b_off), int(b_off.numel()) - 1, ptr(b_doc), ptr(b_tf), ptr(b_map), b_docs,
                                                int(n_terms), int(n_docs), ptr(term_off), ptr(post_doc), ptr(post_tf), max(P, 1),
                                                stream))
    return term_off, post_doc[:P], post_tf[:P]


def bm25_add_token_ids(ix, doc_ids, tok_off, tok_ids, n_terms, device="cpu", vocab=None, docs_meta=None):
    """The incremental BM25.build_index (indexer/bm25_indexer.py:252-344): a NEW CorpusIndex with the documents of this batch
    that have no bm25_doc_stats row yet added to `ix` (which is left unchanged: an engine bound to it stays valid until it
    rebinds).  doc_ids / tok_off / tok_ids as bm25_index_from_token_ids; token ids below n_terms, n_terms >= ix.n_terms.

      * processed: a document whose doc_id is not in ix.doc_ids, or whose doc_len is 0 there (a urlsDB-only document of
        from_duckdb / from_tables: it keeps its dense index).  Documents with a row are skipped (bm25_indexer.py:157-179) and
        counted in the result's `update_counts`; a document without tokens gets no row.  Duplicate ids raise.
      * the batch's postings come from the from-scratch builder (msr_build_postings on a GPU device), documents numbered by
        ascending doc_id, and join the index's through merge_postings (msr_merge_postings) with both sides renumbered;
        total_docs += added; avg_doc_length and the idf of EVERY term are recomputed as the reference does (:346-369,
        :130-147), with the builders' float64 -> REAL rounding: the tables equal a from-scratch build of the union bit for bit.
      * corpus side: doc_off gets zero-chunk entries for the new documents (attach_chunks then appends their chunk rows);
        emb / chunk_ids are kept; urls / titles / texts are extended from docs_meta {doc_id: (url, title, text)} (None where
        absent); the URL groups are recomputed over the whole corpus.  vocab, when given, replaces ix.vocab.
      * forward index: if `ix` has one (tok_off / tok_ids) the result has one in merged document order -- an added document
        gets its stream, a urlsDB-only document that now gets a row keeps its dense index and gets its new stream, every other
        document keeps its own; if `ix` has none the result has none.
    A shard (doc_base != 0 or n_docs_global != n_docs) is refused: update the whole index, then shard it."""
    import torch
    from .index import _np
    if ix.doc_base != 0 or (ix.n_docs_global and ix.n_docs_global != ix.n_docs):
        raise ValueError("bm25_add_token_ids: the index is a shard; update the whole index, then shard it (CorpusIndex.shard)")
    if ix.term_off is None:
        raise ValueError("bm25_add_token_ids: the index has no postings")
    if int(n_terms) < ix.n_terms:
        raise ValueError(f"bm25_add_token_ids: n_terms {n_terms} < the index's {ix.n_terms} (the vocabulary may grow, not shrink)")
    if docs_meta is not None and ix.urls is None:
        raise ValueError("bm25_add_token_ids: docs_meta given, but the index has no urlsDB columns")
    dev = torch.device(device)
    ids = np.asarray(_np(doc_ids), np.int64)
    if len(np.unique(ids)) != len(ids):
        raise ValueError("duplicate doc_id")
    off = np.asarray(_np(tok_off), np.int64)
    lens = np.diff(off)
    tok = tok_ids if torch.is_tensor(tok_ids) else torch.as_tensor(np.asarray(tok_ids, np.int32))
    if tok.numel() and (int(tok.min()) < 0 or int(tok.max()) >= n_terms):
        raise ValueError("token id outside [0, n_terms)")
    old_ids = np.asarray(_np(ix.doc_ids), np.int64)
    old_len = np.asarray(_np(ix.doc_len), np.int32)
    pos = np.minimum(np.searchsorted(old_ids, ids), max(len(old_ids) - 1, 0))
    known = (old_ids[pos] == ids) if len(old_ids) else np.zeros(len(ids), bool)
    has_row = known & (old_len[pos] > 0 if len(old_ids) else known)
    sel = np.nonzero(~has_row & (lens > 0))[0]
    # the batch's own tables (documents 0 .. Nb-1 in ascending doc_id): the from-scratch builder on its tokens
    s_off = np.zeros(len(sel) + 1, np.int64)
    s_off[1:] = np.cumsum(lens[sel])
    src = np.repeat(off[sel] - s_off[:-1], lens[sel]) + np.arange(s_off[-1])
    nb = bm25_index_from_token_ids(ids[sel], s_off, tok[torch.as_tensor(src, device=tok.device)], int(n_terms), device=dev,
                                   keep_tokens=ix.tok_off is not None)
    b_ids = np.asarray(nb.doc_ids, np.int64)
    merged = np.union1d(old_ids, b_ids)
    M = len(merged)
    a_idx = np.searchsorted(merged, old_ids)
    identity = np.array_equal(a_idx, np.arange(len(old_ids)))
    b_map = np.searchsorted(merged, b_ids).astype(np.int32)
    term_off, post_doc, post_tf = merge_postings(ix.term_off, ix.post_doc, ix.post_tf, None if identity else a_idx.astype(np.int32),
                                                 nb.term_off, nb.post_doc, nb.post_tf, b_map, int(n_terms), M, device=dev,
                                                 a_docs=len(old_ids))
    doc_len = np.zeros(M, np.int32)
    doc_len[a_idx] = old_len
    doc_len[b_map] = np.asarray(_np(nb.doc_len), np.int32)
    added = len(b_ids)
    total_docs = int(ix.total_docs) + added
    rows = doc_len[doc_len > 0]
    avgdl = float(np.float32(rows.astype(np.float64).mean())) if len(rows) else 0.0
    idf = idf_real(total_docs, np.diff(np.asarray(_np(term_off), np.int64)))
    out = CorpusIndex(doc_ids=merged, doc_len=torch.as_tensor(doc_len).to(dev), term_off=term_off, post_doc=post_doc,
                      post_tf=post_tf, idf=torch.as_tensor(idf).to(dev), avgdl=avgdl, total_docs=total_docs, k1=ix.k1, b=ix.b,
                      vocab=vocab if vocab is not None else ix.vocab, chunk_ids=ix.chunk_ids, emb=ix.emb)
    out.n_docs_global = M
    if ix.tok_off is not None:                               # both sides' streams side by side, gathered into merged order
        a_off, b_off = np.asarray(_np(ix.tok_off), np.int64), np.asarray(_np(nb.tok_off), np.int64)
        a_tok = (ix.tok_ids if torch.is_tensor(ix.tok_ids) else torch.as_tensor(np.asarray(ix.tok_ids, np.int32))).to(dev, torch.int32)
        src_doc = np.full(M, -1, np.int64)                   # index into the concatenated offsets [a's documents, b's documents]
        src_doc[a_idx] = np.arange(len(old_ids))
        src_doc[b_map] = len(old_ids) + np.arange(len(b_ids))               # (a document on both sides: its new stream)
        starts = np.concatenate([a_off[:-1], a_off[-1] + b_off[:-1]])
        ends = np.concatenate([a_off[1:], a_off[-1] + b_off[1:]])
        lens_m = (ends - starts)[src_doc]
        m_off = np.zeros(M + 1, np.int64)
        m_off[1:] = np.cumsum(lens_m)
        src = np.repeat(starts[src_doc] - m_off[:-1], lens_m) + np.arange(m_off[-1])
        both_tok = torch.cat([a_tok, nb.tok_ids.to(dev, torch.int32)])
        out.tok_off = torch.as_tensor(m_off).to(dev)
        out.tok_ids = both_tok[torch.as_tensor(src, device=both_tok.device)].contiguous()
    if ix.doc_off is not None:
        cnt = np.zeros(M, np.int64)
        cnt[a_idx] = np.diff(np.asarray(_np(ix.doc_off), np.int64))
        doc_off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
        out.doc_off = torch.as_tensor(doc_off).to(ix.doc_off.device) if torch.is_tensor(ix.doc_off) else doc_off
    if ix.urls is not None:
        meta = docs_meta or {}
        new = ~np.isin(b_ids, old_ids)
        for j, name in enumerate(("urls", "titles", "texts")):
            old = getattr(ix, name)
            if old is None:
                continue
            col = [None] * M
            for i, v in zip(a_idx.tolist(), old):
                col[i] = v
            for i, d in zip(b_map[new].tolist(), b_ids[new].tolist()):
                m = meta.get(d)
                col[i] = m[j] if m is not None else None
            setattr(out, name, col)
    out.update_counts = dict(added=added, already_indexed=int(has_row.sum()), no_tokens=int((~has_row & (lens == 0)).sum()))
    return out


def compact_postings(term_off, post_doc, post_tf, keep, device="cpu"):
    """A CSR-by-term posting table without the postings of some documents (msr_compact_postings on a GPU device; a torch
    restatement on the CPU, the reference the GPU tests compare against).  term_off int64 [n_terms + 1], post_doc / post_tf
    int32 (documents ascending inside a term), keep [n_docs] (nonzero / True = the document stays).  A kept document's new
    index is the number of kept documents before it.  Returns (term_off int64 [n_terms + 1], post_doc int32, post_tf int32)
    tensors on `device`: the kept postings in their order, renumbered.  A term_off that is not monotone from 0 or a document
    index outside [0, n_docs) raises (ValueError on the CPU, MsrError on the GPU)."""
    import torch
    dev = torch.device(device)
    if dev.type == "cuda":
        return _compact_postings_hip(term_off, post_doc, post_tf, keep, dev)
    as_t = lambda x, dt: (x if torch.is_tensor(x) else torch.as_tensor(np.ascontiguousarray(x))).to(dev, dt)
    off = as_t(term_off, torch.int64)
    kp = as_t(keep, torch.bool)
    if off.numel() == 0 or int(off[0]) != 0 or bool((off[1:] < off[:-1]).any()):
        raise ValueError("term_off is not a monotone offset array from 0")
    P = int(off[-1])
    doc = as_t(post_doc, torch.int64)[:P]
    tf = as_t(post_tf, torch.int32)[:P]
    if doc.numel() and (int(doc.min()) < 0 or int(doc.max()) >= kp.numel()):
        raise ValueError("a posting's document index is outside [0, n_docs)")
    new = torch.cumsum(kp, 0) - kp.to(torch.int64)                          # kept documents before each document
    kept = kp[doc]
    before = torch.zeros(P + 1, dtype=torch.int64, device=dev)
    before[1:] = torch.cumsum(kept, 0)
    return before[off], new[doc[kept]].to(torch.int32), tf[kept]


def _compact_postings_hip(term_off, post_doc, post_tf, keep, dev):
    """compact_postings through the C ABI (msr_compact_postings); no fallback."""
    import ctypes as C

    import torch

    from . import _abi
    lib = _abi.load()
    on_dev = lambda x, dt: (x if torch.is_tensor(x) else torch.as_tensor(np.ascontiguousarray(x))).to(dev, dt).contiguous()
    off, doc, tf = on_dev(term_off, torch.int64), on_dev(post_doc, torch.int32), on_dev(post_tf, torch.int32)
    kp = on_dev(keep, torch.bool).to(torch.uint8)
    n_terms = int(off.numel()) - 1
    out_off = torch.empty(n_terms + 1, dtype=torch.int64, device=dev)
    n_post = C.c_int64(0)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else C.c_void_p(0)
    P = int(off[-1].item()) if n_terms >= 0 else 0
    if P > min(doc.numel(), tf.numel()):
        raise ValueError(f"term_off[-1] = {P} postings, but post_doc / post_tf hold {min(doc.numel(), tf.numel())}")
    # one call, sized by the input (the kept postings are at most P): no sizing call and no second counting pass
    out_doc = torch.empty(max(P, 1), dtype=torch.int32, device=dev)
    out_tf = torch.empty(max(P, 1), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _abi.check(None, lib.msr_compact_postings(ptr(off), n_terms, ptr(doc), ptr(tf), ptr(kp), int(kp.numel()), ptr(out_off),
                                                  ptr(out_doc), ptr(out_tf), max(P, 1), C.byref(n_post), stream))
    K = int(n_post.value)
    return out_off, out_doc[:K], out_tf[:K]


def remove_documents(ix, doc_ids, device="cpu"):
    """A NEW CorpusIndex without the documents `doc_ids` (`ix` is left unchanged: an engine bound to it stays valid until it
    rebinds).  The counterpart of bm25_add_token_ids; a document that changed is replaced by removing it and adding its new
    version under the same doc_id.

      * every listed document the index has goes, urlsDB-only documents (doc_len 0) included: from doc_ids / doc_len, the
        postings (compact_postings: msr_compact_postings on a GPU device), the chunk rows (doc_off / chunk_ids / emb, gathered
        on emb's own device), urls / titles / texts; the kept documents keep their order and are renumbered densely; the
        URL groups are recomputed; a forward index (tok_off / tok_ids) is gathered to the kept documents' streams.
      * total_docs -= the removed documents that had a BM25 row; avg_doc_length and the idf of EVERY term are recomputed
        with the builders' float64 -> REAL rounding (n_terms stays: a term left without postings gets the idf a
        from-scratch build gives it), so the tables equal a from-scratch build of the remaining documents bit for bit.
      * ids the index does not have are counted, not raised; a duplicate id raises.  `update_counts` = dict(removed,
        removed_rows, not_found).
    A shard (doc_base != 0 or n_docs_global != n_docs) is refused: remove from the whole index, then shard it."""
    import torch
    from .index import _np
    if ix.doc_base != 0 or (ix.n_docs_global and ix.n_docs_global != ix.n_docs):
        raise ValueError("remove_documents: the index is a shard; remove from the whole index, then shard it (CorpusIndex.shard)")
    dev = torch.device(device)
    ids = np.asarray(_np(doc_ids), np.int64).reshape(-1)
    if len(np.unique(ids)) != len(ids):
        raise ValueError("duplicate doc_id")
    old_ids = np.asarray(_np(ix.doc_ids), np.int64)
    N = len(old_ids)
    pos = np.minimum(np.searchsorted(old_ids, ids), max(N - 1, 0))
    found = (old_ids[pos] == ids) if N else np.zeros(len(ids), bool)
    keep = np.ones(N, bool)
    keep[pos[found]] = False
    old_len = None if ix.doc_len is None else np.asarray(_np(ix.doc_len), np.int32)
    removed_rows = int((old_len[~keep] > 0).sum()) if old_len is not None else 0
    out = CorpusIndex(doc_ids=old_ids[keep], avgdl=ix.avgdl, total_docs=int(ix.total_docs) - removed_rows, k1=ix.k1, b=ix.b,
                      vocab=ix.vocab)
    out.n_docs_global = out.n_docs
    if old_len is not None:
        doc_len = old_len[keep]
        rows = doc_len[doc_len > 0]
        out.avgdl = float(np.float32(rows.astype(np.float64).mean())) if len(rows) else 0.0
        out.doc_len = torch.as_tensor(doc_len).to(dev)
    if ix.term_off is not None:
        out.term_off, out.post_doc, out.post_tf = compact_postings(ix.term_off, ix.post_doc, ix.post_tf, keep, device=dev)
        out.idf = torch.as_tensor(idf_real(out.total_docs, np.diff(np.asarray(_np(out.term_off), np.int64)))).to(dev)
    if ix.doc_off is not None:
        cnt = np.diff(np.asarray(_np(ix.doc_off), np.int64))
        doc_off = np.concatenate([[0], np.cumsum(cnt[keep])]).astype(np.int32)
        out.doc_off = torch.as_tensor(doc_off).to(ix.doc_off.device) if torch.is_tensor(ix.doc_off) else doc_off
        rows = np.repeat(keep, cnt)
        if ix.chunk_ids is not None:
            out.chunk_ids = np.asarray(_np(ix.chunk_ids), np.int64)[rows]
        if torch.is_tensor(ix.emb):
            out.emb = ix.emb.index_select(0, torch.as_tensor(np.nonzero(rows)[0], device=ix.emb.device))
        elif ix.emb is not None:
            out.emb = np.asarray(ix.emb)[rows]
    if ix.tok_off is not None:
        tok = ix.tok_ids if torch.is_tensor(ix.tok_ids) else torch.as_tensor(np.asarray(ix.tok_ids, np.int32))
        k_off, k_tok = _gather_streams(ix.tok_off, tok.to(dev, torch.int32), np.nonzero(keep)[0])
        out.tok_off, out.tok_ids = torch.as_tensor(k_off).to(dev), k_tok
    for name in ("urls", "titles", "texts"):
        col = getattr(ix, name)
        if col is not None:
            setattr(out, name, [v for v, k in zip(col, keep.tolist()) if k])
    out.update_counts = dict(removed=int(found.sum()), removed_rows=removed_rows, not_found=int((~found).sum()))
    return out


# ---------------------------------------------------------------------------------------------------------------- forward index
def attach_tokens(ix, tok_off, tok_ids):
    """Give an index that came without a forward index (CorpusIndex.from_tables / from_duckdb, a loaded snapshot, a build
    without keep_tokens) the token streams phrase search reads: tok_off int64 [N+1], tok_ids int32 [T], document i's stream
    (the ids it was indexed from, in the index's dense document order) at tok_ids[tok_off[i]:tok_off[i+1]].  Validated here,
    ValueError otherwise: N + 1 offsets that start at 0, ascend and end at len(tok_ids); ids in [0, n_terms); every document's
    length equals its doc_len (a document without a BM25 row has length 0).  Sets ix.tok_off / ix.tok_ids and returns ix; an
    engine already bound to ix sees them after DeviceEngine.rebind / Retriever.update_index.  CorpusIndex.save / load keep
    them; save_dir / load_dir and shard drop them."""
    import torch
    from .index import _np
    off = np.asarray(_np(tok_off)).reshape(-1)
    ids = np.asarray(_np(tok_ids)).reshape(-1)
    N = ix.n_docs
    if len(off) != N + 1:
        raise ValueError(f"attach_tokens: {len(off)} offsets for an index of {N} documents (N + 1 = {N + 1} are needed)")
    if not np.issubdtype(off.dtype, np.integer) or (len(ids) and not np.issubdtype(ids.dtype, np.integer)):
        raise ValueError("attach_tokens: offsets and ids are integers")
    off = off.astype(np.int64)
    if off[0] != 0:
        raise ValueError("attach_tokens: tok_off[0] must be 0")
    if (np.diff(off) < 0).any():
        raise ValueError("attach_tokens: tok_off descends")
    if off[-1] != len(ids):
        raise ValueError(f"attach_tokens: tok_off ends at {int(off[-1])}, tok_ids holds {len(ids)} ids")
    if len(ids) and (int(ids.min()) < 0 or int(ids.max()) >= ix.n_terms):
        raise ValueError(f"attach_tokens: a token id is outside [0, n_terms = {ix.n_terms})")
    want = np.zeros(N, np.int64) if ix.doc_len is None else np.asarray(_np(ix.doc_len), np.int64)
    bad = np.nonzero(np.diff(off) != want)[0]
    if len(bad):
        d = int(bad[0])
        raise ValueError(f"attach_tokens: document {d} has {int(off[d + 1] - off[d])} tokens, its doc_len is {int(want[d])}")
    if torch.is_tensor(tok_ids):
        ix.tok_off, ix.tok_ids = torch.as_tensor(off).to(tok_ids.device), tok_ids.to(torch.int32).reshape(-1).contiguous()
    else:
        ix.tok_off, ix.tok_ids = off, ids.astype(np.int32)
    return ix


def tokens_from_texts(ix, tokenizer=None):
    """(tok_off int64 [N+1], tok_ids int32 [T]) for attach_tokens, from the index's own titles / texts: every document's
    normalise_document_text(title, text) through `tokenizer` (default text.simple_tokenize; it must be the tokenizer the index
    was built with) and ix.vocab.  ValueError if the index has no texts or vocabulary, a token is not in the vocabulary, or a
    document's token count differs from its doc_len (a document without a BM25 row must tokenise to nothing)."""
    from .index import _np
    from .text import simple_tokenize
    tok = tokenizer or simple_tokenize
    if ix.texts is None or ix.vocab is None:
        raise ValueError("tokens_from_texts: the index needs texts and a vocabulary")
    N = ix.n_docs
    want = np.zeros(N, np.int64) if ix.doc_len is None else np.asarray(_np(ix.doc_len), np.int64)
    titles = ix.titles if ix.titles is not None else [None] * N
    off, ids, vocab = np.zeros(N + 1, np.int64), [], ix.vocab
    for d in range(N):
        words = tok(normalise_document_text(titles[d], ix.texts[d]))
        if len(words) != want[d]:
            raise ValueError(f"tokens_from_texts: document {d} tokenises to {len(words)} tokens, its doc_len is {int(want[d])}")
        for w in words:
            t = vocab.get(w)
            if t is None:
                raise ValueError(f"tokens_from_texts: token {w!r} of document {d} is not in the vocabulary")
            ids.append(t)
        off[d + 1] = len(ids)
    return off, np.asarray(ids, np.int32)
