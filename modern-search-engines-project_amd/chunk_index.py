"""Documents -> chunk rows of the dense index (the corpus side of the reference: indexer/indexer.py:95-110,157-172,
`Indexer.index_documents`).

    table = embed_documents(encoder, docs, first_chunk_id=0)       # plan_chunks + QueryEncoder.encode_chunks
    ix = attach_chunks(bm25_index_from_token_ids(...), table)       # rows in the order CorpusIndex requires

The reference, per document in ascending id order: full_text = f"{title or ''} {text or ''}".strip() (empty: no chunk);
tokens without special tokens; sliding windows of 512 tokens, step 450 (config.py:10-11, embedder.py:65-87); each window
decoded back to text (skip_special_tokens) and encoded by the bi-encoder with normalize_embeddings=True, which tokenises
it again WITH [CLS] / [SEP].  Chunk ids run on from MAX(chunk_id) + 1 in document order, then window order.  Planning is
host-only; the encoding is the HIP forward pass of encoder.py (msr_enc_attention_long for the attention).
"""
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

from .index import DIM, _np
from .text import create_sliding_windows

WINDOW_SIZE, STEP_SIZE = 512, 450                           # config.py:10-11


@dataclass
class ChunkTable:
    chunk_ids: np.ndarray                                   # int64 [C], ascending
    doc_ids: np.ndarray                                     # int64 [C]: the owning document of every chunk
    seqs: List[List[int]]                                   # token ids the encoder takes (special tokens included)
    texts: Optional[List[str]] = None                       # chunks_optimized.chunk_text (text input only)
    emb: object = None                                      # float32 [C, 768] device tensor, unit rows (embed_documents)

    def __len__(self):
        return len(self.chunk_ids)

    @property
    def next_chunk_id(self):
        """The first_chunk_id of a later call that appends documents (MAX(chunk_id) + 1)."""
        return int(self.chunk_ids[-1]) + 1 if len(self.chunk_ids) else None


def plan_chunks(docs, tokenizer=None, window_size=WINDOW_SIZE, step_size=STEP_SIZE, first_chunk_id=0, cls_id=None,
                sep_id=None):
    """docs: (doc_id, title, text) triples -- cut as indexer.py:95-110 does, with `tokenizer` (a tokenizers.Tokenizer,
    e.g. QueryEncoder.tokenizer) -- or (doc_id, token_ids) pairs, windowed as given and wrapped in cls_id / sep_id when
    those are given (a document without tokens gets no chunk).  Returns a ChunkTable without embeddings; chunk ids run
    from first_chunk_id in ascending doc_id order, then window order."""
    docs = sorted(docs, key=lambda d: int(d[0]))
    ids = [int(d[0]) for d in docs]
    if len(set(ids)) != len(ids):
        raise ValueError("duplicate doc_id")
    chunk_doc, seqs, texts = [], [], []
    text_mode = None
    for d in docs:
        is_text = len(d) == 3
        if text_mode is None:
            text_mode = is_text
        elif text_mode != is_text:
            raise ValueError("docs mixes (doc_id, title, text) and (doc_id, token_ids) entries")
        if is_text:
            if tokenizer is None:
                raise ValueError("text documents need a tokenizer")
            full_text = f"{d[1] or ''} {d[2] or ''}".strip()
            if not full_text:
                continue
            tokens = tokenizer.encode(full_text, add_special_tokens=False).ids
            for w in create_sliding_windows(tokens, window_size=window_size, step_size=step_size):
                chunk_text = tokenizer.decode(w, skip_special_tokens=True)
                texts.append(chunk_text)
                seqs.append(list(tokenizer.encode(chunk_text).ids))
                chunk_doc.append(int(d[0]))
        else:
            tokens = [int(t) for t in d[1]]
            if not tokens:
                continue
            for w in create_sliding_windows(tokens, window_size=window_size, step_size=step_size):
                seqs.append(([cls_id] if cls_id is not None else []) + list(w) + ([sep_id] if sep_id is not None else []))
                chunk_doc.append(int(d[0]))
    C = len(seqs)
    return ChunkTable(chunk_ids=np.arange(first_chunk_id, first_chunk_id + C, dtype=np.int64),
                      doc_ids=np.array(chunk_doc, np.int64), seqs=seqs, texts=texts if text_mode else None)


def embed_documents(encoder, docs, tokenizer=None, window_size=WINDOW_SIZE, step_size=STEP_SIZE, first_chunk_id=0,
                    cls_id=None, sep_id=None, batch_tokens=None):
    """plan_chunks, then every chunk through encoder.encode_chunks (normalize_embeddings=True, indexer.py:165): the table
    with emb = unit-norm float32 [C, 768] rows on the encoder's device, row i = chunk_ids[i]."""
    import torch
    if tokenizer is None:
        tokenizer = encoder.tokenizer
    table = plan_chunks(docs, tokenizer=tokenizer, window_size=window_size, step_size=step_size,
                        first_chunk_id=first_chunk_id, cls_id=cls_id, sep_id=sep_id)
    emb = torch.zeros((len(table), DIM), dtype=torch.float32, device=encoder.device)
    kw = {} if batch_tokens is None else {"batch_tokens": int(batch_tokens)}
    encoder.encode_chunks(table.seqs, normalize=True, out=emb, **kw)
    table.emb = emb
    return table


def attach_chunks(ix, *tables):
    """Put chunk tables into a CorpusIndex (e.g. one of index_build.bm25_index_from_token_ids) in the layout it requires:
    rows sorted by (dense document index, chunk_id), doc_off [N+1] the row range of every document.  Rows the index
    already has are kept, so a table of later documents (first_chunk_id = the previous table's next_chunk_id) appends
    to it.  Every chunk's document must be a document of the index; chunk ids must be unique.  Returns ix."""
    import torch
    doc_ids = np.asarray(_np(ix.doc_ids), np.int64)
    cids, owners, embs = [], [], []
    if ix.doc_off is not None and ix.chunk_ids is not None and ix.emb is not None:
        off = np.asarray(_np(ix.doc_off), np.int64)
        cids.append(np.asarray(_np(ix.chunk_ids), np.int64))
        owners.append(np.repeat(doc_ids, np.diff(off)))
        embs.append(ix.emb)
    for t in tables:
        if t.emb is None:
            raise ValueError("the chunk table has no embeddings (embed_documents fills them)")
        cids.append(np.asarray(t.chunk_ids, np.int64))
        owners.append(np.asarray(t.doc_ids, np.int64))
        embs.append(t.emb)
    cid = np.concatenate(cids) if cids else np.zeros(0, np.int64)
    own = np.concatenate(owners) if owners else np.zeros(0, np.int64)
    if len(np.unique(cid)) != len(cid):
        raise ValueError("duplicate chunk_id")
    rank = np.searchsorted(doc_ids, own)
    if len(own) and (np.any(rank >= len(doc_ids)) or np.any(doc_ids[np.minimum(rank, len(doc_ids) - 1)] != own)):
        raise ValueError("a chunk belongs to a document the index does not have")
    order = np.lexsort((cid, rank))
    dev = next((e.device for e in embs if isinstance(e, torch.Tensor)), torch.device("cpu"))
    emb = torch.cat([torch.as_tensor(e, dtype=torch.float32).to(dev).reshape(-1, DIM) for e in embs]) if embs else \
        torch.zeros((0, DIM), dtype=torch.float32, device=dev)
    ix.emb = emb[torch.as_tensor(order, device=dev)].contiguous()
    ix.chunk_ids = cid[order]
    ix.doc_off = np.concatenate([[0], np.cumsum(np.bincount(rank, minlength=len(doc_ids)))]).astype(np.int32)
    return ix
