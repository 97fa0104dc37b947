#!/usr/bin/env python3
"""End-to-end drop-in demo (BASELINE configs[0] shape): answer the reference's queries.txt format with the
two-stage path and write `qnum<TAB>rank<TAB>url<TAB>score` lines, like POST /api/batch_search_file
(search_api.py:331-367).  The reference's crawl database is not available offline, so a small synthetic "crawl"
is generated: documents are bags of words from a vocabulary that contains the query words, indexed with
msretr.index_build (the reference's BM25.build_index semantics) and given random unit-norm chunk embeddings.

    python examples/run_queries_txt.py [--fuzzy] [--wildcards] [--collapse-duplicates] [--match VALUE] [queries.txt] [out.txt]

--fuzzy: words the vocabulary lacks are replaced by their nearest term (Retriever.batch_search(fuzzy=True)) and every
correction is printed.
--wildcards: `bibliothek*`, `*bibliothek`, `t?bingen` are expanded over the vocabulary
(Retriever.batch_search(wildcards=True)) and every expansion is printed.
--collapse-duplicates: every tenth page of the crawl is a mirror of the page before it under another host; near-duplicate
pages are shown once (Retriever.batch_search(collapse_duplicates=True)) and the number of rows dropped per query is printed.
--match all | 2 | 75%: only pages that hold all / at least two / three quarters of a query's words
(Retriever.batch_search(match=...)); every query's slots and how many of them a page must fill are printed.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from msretr.index_build import bm25_index_from_tokens  # noqa: E402
from msretr.text import preprocess_query, read_queries_file, simple_tokenize  # noqa: E402

DEFAULT_QUERIES = ["tübingen attractions", "food and drinks", "university tuebingen research programs",
                   "castle hohentubingen history", "botanical garden opening hours"]     # shape of queries.txt:1-5


def synthetic_crawl(n_docs=3000, seed=7, queries=DEFAULT_QUERIES, mirrors=False):
    rng = np.random.default_rng(seed)
    words = sorted({w for q in queries for w in simple_tokenize(preprocess_query(q))})
    filler = [f"wort{i}" for i in range(400)]
    vocab = words + filler
    p = 1.0 / np.arange(1, len(filler) + 1) ** 0.8
    p = np.r_[np.full(len(words), 0.0035), 0.95 * p / p.sum()]      # a query word is in ~1/3 of the documents
    p /= p.sum()
    doc_ids = (np.cumsum(rng.integers(1, 4, size=n_docs)) + 10).tolist()
    tokens, urls, titles, texts = [], [], [], []
    for i, d in enumerate(doc_ids):
        n = int(rng.integers(20, 200))
        toks = [vocab[j] for j in rng.choice(len(vocab), size=n, p=p)]
        if rng.random() < 0.85:
            toks[0] = "tübingen"
        if mirrors and i % 10 == 9:
            toks = list(tokens[-1])                          # the page before, once more, under another host
        tokens.append(toks)
        urls.append(f"https://www.site{int(d) % 53}.de/page/{int(d)}" + ("?ref=1" if d % 19 == 0 else ""))
        titles.append(f"Seite {int(d)}")
        texts.append(" ".join(toks))
    ix = bm25_index_from_tokens(doc_ids, tokens, keep_tokens=mirrors)     # (the collapse reads the forward index)
    ix.urls, ix.titles, ix.texts = urls, titles, texts
    cnt = rng.integers(1, 9, size=len(doc_ids))
    ix.doc_off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    C = int(ix.doc_off[-1])
    ix.chunk_ids = np.arange(C, dtype=np.int64)
    emb = rng.standard_normal((C, 768)).astype(np.float32)
    ix.emb = emb / np.linalg.norm(emb, axis=1, keepdims=True)
    return ix


def fake_encoder(dim=768):
    """Stand-in for the sentence encoder (the reference loads a HF model by name): a seeded hash of the text."""
    def enc(text):
        r = np.random.default_rng(abs(hash(text)) % (2 ** 32))
        return (r.standard_normal(dim) * 3).astype(np.float32)
    return enc


def main():
    from msretr.retriever import Retriever
    args, match = sys.argv[1:], "any"
    if "--match" in args:                                    # --match all | --match 2 | --match 75%
        at = args.index("--match")
        if at + 1 >= len(args):
            sys.exit("--match needs a value: all, a whole number, or a percentage like 75%")
        match = args[at + 1]
        match = int(match) if match.lstrip("-").isdigit() else match
        del args[at:at + 2]
    argv = [a for a in args if a not in ("--fuzzy", "--wildcards", "--collapse-duplicates")]
    fuzzy, wildcards = "--fuzzy" in sys.argv[1:], "--wildcards" in sys.argv[1:]
    collapse = "--collapse-duplicates" in sys.argv[1:]
    qfile = argv[0] if len(argv) > 0 else None
    out = argv[1] if len(argv) > 1 else "batch_search_results.txt"
    queries = read_queries_file(qfile) if qfile else [(str(i + 1), q) for i, q in enumerate(DEFAULT_QUERIES)]
    ix = synthetic_crawl(mirrors=collapse)
    rt = Retriever(embedder=fake_encoder(), indexer=ix, tokenizer=simple_tokenize, max_queries=8, max_k=1000)
    # the reference's `results` list (dicts built on access) ...
    res = rt.batch_search(queries, fuzzy=fuzzy, wildcards=wildcards, collapse_duplicates=collapse, match=match)
    res.write(out)                                  # ... and all formatted lines in one native call
    print(f"{len(queries)} queries -> {len(res)} result lines in {out}")
    for (qn, _), text in zip(queries, res.corrected_queries or ()):
        if text is not None:
            print(f"query {qn}: searched for {text!r}")
    for (qn, _), exp in zip(queries, res.expansions or ()):
        for pattern, info in exp.items():
            print(f"query {qn}: {pattern} -> {', '.join(info['terms']) or 'nothing'} ({info['total']} matches)")
    for (qn, _), m in zip(queries, res.match or ()):
        print(f"query {qn}: pages that hold at least {m['need']} of {' | '.join('/'.join(map(str, s)) for s in m['slots'])}")
    for (qn, _), dropped in zip(queries, res.collapsed or ()):
        print(f"query {qn}: {dropped} near-duplicate rows collapsed")
    rt.engine.close()


if __name__ == "__main__":
    main()
