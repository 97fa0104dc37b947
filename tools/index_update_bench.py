#!/usr/bin/env python3
"""Time adding documents to and removing them from a built index (index_build.bm25_add_token_ids, msr_merge_postings,
index_build.remove_documents, msr_compact_postings, DeviceEngine.rebind).

    python tools/index_update_bench.py [--rows build,merge,rebind,remove] [--reps 5]

Four rows, one JSON line each (remove: one per pattern):
  build   the build_index_bench.py corpus (200 k documents, 200 k terms) plus 2 k / 20 k new documents (ids above the old ones):
          the whole update on the GPU and its parts -- the new documents' tables (msr_build_postings), the merge, the host idf.
  merge   the headline shape: a 1 M-document index of ~2.35e8 postings (synthetic.synthetic_corpus) plus 1 % new documents
          (10 k, ~2.35e6 postings), appended ids (A keeps its indices) and interleaved ids (both sides renumbered): the
          msr_merge_postings call, with the bytes it must move (read doc + tf of both sides, write the merged doc + tf, the
          map lookups).  Kernel times and the effective bandwidth come from a rocprofv3 --kernel-trace --stats run of this row.
  rebind  a 200 k-document index with 1 M chunk rows bound to a DeviceEngine(max_queries=256), grown by 2 k documents and
          their chunks: rebind split into postings and chunks (the chunk bind includes the fragment-order copy), and the
          device memory in use before and after (both indices resident).
  remove  the merge row's index (the same seed: ~2.37e8 postings) with 5 M chunk rows; 1 % of the documents removed, scattered
          and as one contiguous block: the msr_compact_postings call with the bytes it must move (the counting pass reads
          doc, the write pass reads doc + tf and writes the kept doc + tf, term_off read and written), the whole
          remove_documents, its chunk-row gather alone (index_select of the kept rows: read + write), and the rebind of a
          DeviceEngine(max_queries=256) from the old index to the new one.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from msretr.index_build import (bm25_add_token_ids, bm25_index_from_token_ids, compact_postings, idf_real,  # noqa: E402
                                merge_postings, remove_documents)


def sync_time(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return out, float(np.median(ts)) * 1e3


def tokens(rng, ids, mean_len, terms):
    lens = np.clip(rng.lognormal(np.log(mean_len) - 0.32, 0.8, size=len(ids)), 8, 20000).astype(np.int64)
    off = np.zeros(len(ids) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    return ids, off, (rng.zipf(1.07, size=int(off[-1])) % terms).astype(np.int32)


def row_build(reps):
    rng = np.random.default_rng(3)
    base = tokens(rng, np.arange(200_000, dtype=np.int64) * 2 + 1, 370, 200_000)
    ix = bm25_index_from_token_ids(*base, 200_000, device="cuda")
    for n_new in (2_000, 20_000):
        upd = tokens(rng, np.arange(n_new, dtype=np.int64) * 2 + 400_001, 370, 200_000)
        new, t_all = sync_time(lambda: bm25_add_token_ids(ix, *upd, 200_000, device="cuda"), reps)
        nb, t_build = sync_time(lambda: bm25_index_from_token_ids(*upd, 200_000, device="cuda"), reps)
        b_map = np.arange(200_000, 200_000 + n_new, dtype=np.int32)
        _, t_merge = sync_time(lambda: merge_postings(ix.term_off, ix.post_doc, ix.post_tf, None, nb.term_off, nb.post_doc,
                                                      nb.post_tf, b_map, 200_000, 200_000 + n_new, device="cuda",
                                                      a_docs=200_000), reps)
        df = np.diff(new.term_off.cpu().numpy())
        _, t_idf = sync_time(lambda: idf_real(new.total_docs, df), reps)
        print(json.dumps({"row": "build", "docs": 200_000, "new_docs": n_new, "postings": int(new.post_doc.numel()),
                          "new_postings": int(nb.post_doc.numel()), "update_ms": round(t_all, 2), "new_docs_build_ms": round(t_build, 2),
                          "merge_ms": round(t_merge, 2), "host_idf_ms": round(t_idf, 2),
                          "rest_ms": round(t_all - t_build - t_merge - t_idf, 2)}), flush=True)


def row_merge(reps):
    from msretr.synthetic import synthetic_corpus
    a = synthetic_corpus(1_000_000, n_chunks=0, device="cuda", seed=5)
    b = synthetic_corpus(10_000, n_chunks=0, n_terms=1_000_000, device="cuda", seed=6)
    na, nb, V = a.n_docs, b.n_docs, a.n_terms
    rng = np.random.default_rng(8)
    for pattern in ("appended", "interleaved"):
        if pattern == "appended":
            a_map, b_map = None, np.arange(na, na + nb, dtype=np.int32)
        else:
            b_map = np.sort(rng.choice(na + nb, nb, replace=False)).astype(np.int32)
            a_map = np.setdiff1d(np.arange(na + nb), b_map).astype(np.int32)
        am = None if a_map is None else torch.as_tensor(a_map, device="cuda")
        bm = torch.as_tensor(b_map, device="cuda")
        out, t = sync_time(lambda: merge_postings(a.term_off, a.post_doc, a.post_tf, am, b.term_off, b.post_doc, b.post_tf, bm, V,
                                                  na + nb, device="cuda", a_docs=na), reps)
        P = int(out[1].numel())
        moved = 16 * P + 4 * P * (1 if a_map is not None else 0) + 4 * int(b.post_doc.numel()) + 8 * 2 * (V + 1)
        print(json.dumps({"row": "merge", "pattern": pattern, "docs": na, "new_docs": nb, "postings": P,
                          "new_postings": int(b.post_doc.numel()), "terms": V, "call_ms": round(t, 3), "bytes_moved": moved,
                          "call_effective_TBps": round(moved / (t * 1e-3) / 1e12, 3)}), flush=True)
        del out


def row_rebind(reps):
    from msretr.chunk_index import ChunkTable, attach_chunks
    from msretr.engine import DeviceEngine
    from msretr.index import CorpusIndex
    rng = np.random.default_rng(4)
    base_tok = tokens(rng, np.arange(200_000, dtype=np.int64) * 2 + 1, 370, 200_000)
    upd_tok = tokens(rng, np.arange(2_000, dtype=np.int64) * 2 + 400_001, 370, 200_000)

    def table(ids, first):
        own = np.repeat(ids, 5)
        e = torch.randn((len(own), 768), device="cuda")
        e /= e.norm(dim=1, keepdim=True)
        return ChunkTable(chunk_ids=np.arange(first, first + len(own), dtype=np.int64), doc_ids=own, seqs=[], emb=e)
    t0 = table(base_tok[0], 0)
    base = attach_chunks(bm25_index_from_token_ids(*base_tok, 200_000, device="cuda"), t0)
    grown = attach_chunks(bm25_add_token_ids(base, *upd_tok, 200_000, device="cuda"), table(upd_tok[0], len(t0)))
    post_only = CorpusIndex(doc_ids=grown.doc_ids, doc_len=grown.doc_len, term_off=grown.term_off, post_doc=grown.post_doc,
                            post_tf=grown.post_tf, idf=grown.idf, avgdl=grown.avgdl, total_docs=grown.total_docs)
    eng = DeviceEngine(base, max_queries=256)
    torch.cuda.synchronize()
    used = lambda: (lambda f, t: t - f)(*torch.cuda.mem_get_info())
    before, owned_before = used(), eng.owned_bytes()
    t_all, t_post = [], []
    for _ in range(reps):
        eng.rebind(base)
        t = time.perf_counter(); eng.rebind(post_only); t_post.append(time.perf_counter() - t)
        eng.rebind(base)
        t = time.perf_counter(); eng.rebind(grown); t_all.append(time.perf_counter() - t)
    after = used()
    # peak while rebinding: a thread samples the device's used memory every 0.5 ms during one more rebind
    import threading
    eng.rebind(base)
    peak, stop = [0], threading.Event()

    def sample():
        while not stop.is_set():
            peak[0] = max(peak[0], used())
            time.sleep(0.0005)
    th = threading.Thread(target=sample)
    th.start()
    eng.rebind(grown)
    stop.set()
    th.join()
    ta, tp = float(np.median(t_all)) * 1e3, float(np.median(t_post)) * 1e3
    print(json.dumps({"row": "rebind", "docs": base.n_docs, "new_docs": grown.n_docs - base.n_docs, "chunks": grown.n_chunks,
                      "rebind_ms": round(ta, 2), "postings_bind_ms": round(tp, 2), "chunks_bind_ms": round(ta - tp, 2),
                      "row_copy": eng.row_copy_state(), "device_used_bytes_before": before, "device_used_bytes_after": after,
                      "device_used_bytes_peak_sampled": peak[0],
                      "engine_owned_bytes_before": owned_before, "engine_owned_bytes_after": eng.owned_bytes()}), flush=True)
    eng.close()


def row_remove(reps):
    from msretr.engine import DeviceEngine
    from msretr.index import _np
    from msretr.synthetic import synthetic_corpus
    a = synthetic_corpus(1_000_000, n_chunks=5_000_000, device="cuda", seed=5)    # postings: the merge row's A
    N, V, P = a.n_docs, a.n_terms, int(a.post_doc.numel())
    ids = np.asarray(_np(a.doc_ids))
    cnt = np.diff(np.asarray(_np(a.doc_off), np.int64))
    eng = DeviceEngine(a, max_queries=256)
    rng = np.random.default_rng(9)
    for pattern in ("scattered", "block"):
        gone = np.sort(rng.choice(N, N // 100, replace=False)) if pattern == "scattered" else np.arange(N // 2, N // 2 + N // 100)
        keep = np.ones(N, bool)
        keep[gone] = False
        kt = torch.as_tensor(keep, device="cuda")
        out, t_call = sync_time(lambda: compact_postings(a.term_off, a.post_doc, a.post_tf, kt, device="cuda"), reps)
        K = int(out[1].numel())
        moved = 4 * P + 8 * P + 8 * K + 8 * 2 * (V + 1)
        del out
        new, t_all = sync_time(lambda: remove_documents(a, ids[gone], device="cuda"), reps)
        rows = torch.as_tensor(np.nonzero(np.repeat(keep, cnt))[0], device="cuda")
        _, t_gather = sync_time(lambda: a.emb.index_select(0, rows), reps)
        gather_bytes = 2 * int(rows.numel()) * 768 * 4
        t_rebind = []
        for _ in range(max(1, min(reps, 3))):
            eng.rebind(a)
            torch.cuda.synchronize()
            t = time.perf_counter()
            eng.rebind(new)
            torch.cuda.synchronize()
            t_rebind.append(time.perf_counter() - t)
        eng.rebind(a)
        print(json.dumps({"row": "remove", "pattern": pattern, "docs": N, "removed_docs": len(gone), "postings": P, "kept_postings": K,
                          "terms": V, "chunks": a.n_chunks, "kept_chunks": int(rows.numel()), "call_ms": round(t_call, 3),
                          "bytes_moved": moved, "call_effective_TBps": round(moved / (t_call * 1e-3) / 1e12, 3),
                          "remove_documents_ms": round(t_all, 2), "chunk_gather_ms": round(t_gather, 2),
                          "chunk_gather_TBps": round(gather_bytes / (t_gather * 1e-3) / 1e12, 3),
                          "rest_ms": round(t_all - t_call - t_gather, 2), "rebind_ms": round(float(np.median(t_rebind)) * 1e3, 1),
                          "row_copy": eng.row_copy_state()}), flush=True)
        del new
    eng.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="build,merge,rebind,remove")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("index_update_bench.py needs a GPU")
    for r in args.rows.split(","):
        {"build": row_build, "merge": row_merge, "rebind": row_rebind, "remove": row_remove}[r](args.reps)
