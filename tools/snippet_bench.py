#!/usr/bin/env python3
"""Cost of query-biased snippets (msr_best_windows, DESIGN K14) on the corpus, generator and seeds of tools/phrase_bench.py (a
token-stream corpus built on the GPU with keep_tokens=True), with ONE further document of 100 000 tokens appended behind the
generator's draws (document N; the others are what they are in phrase_bench):
  kernel     256 queries x 100 results = 25 600 pairs, span 30, rows of 3 and of 8 terms (the city, then mid-frequency words;
             each query's documents are drawn from the posting list of its first mid-frequency word) -- device events, one
             warm-up, median of --iters with the fastest and the slowest beside it; the byte model (4 bytes per token of the
             pairs' documents + 28 bytes written per pair)
  long       the same pairs with the 100 000-token document in pair 0's place: one wave walks it serially
  host       the same answers with numpy on the host (tests/snippet_ref.best_windows_fast, host clock), asserted equal
  batch      Retriever.search_batch of 256 three-word queries with and without snippets=True on the host clock (pages are
             rendered from the token streams on first access and cached: the timed calls find them as strings), and the
             snippet step alone split into its kernel call, its copies and its rendering
Prints one JSON line.
    python tools/snippet_bench.py [--docs 1000000] [--queries 256] [--results 100] [--iters 10] [--no-batch]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from msretr.engine import DeviceEngine  # noqa: E402
from msretr.index_build import bm25_index_from_token_ids  # noqa: E402
from msretr.retriever import Retriever  # noqa: E402
from msretr.snippets import query_row, render, term_weights  # noqa: E402
from snippet_ref import best_windows_fast  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=1_000_000)
ap.add_argument("--terms", type=int, default=200_000)
ap.add_argument("--mean-len", type=float, default=120.0)
ap.add_argument("--queries", type=int, default=256)
ap.add_argument("--results", type=int, default=100)
ap.add_argument("--span", type=int, default=30)
ap.add_argument("--long-tokens", type=int, default=100_000)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--no-batch", action="store_true")
a = ap.parse_args()
dev = torch.device("cuda", 0)
PEAK_GBS = 6100.0                                            # streaming read the README measures (6.1 TB/s)


def log(*x):
    print(*x, file=sys.stderr, flush=True)


def timed(fn, iters):
    """(median, fastest, slowest) device time (ms) of fn() over iters calls, after one warm-up call."""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ts.append(s.elapsed_time(e))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def host_timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


# ---- the corpus of tools/phrase_bench.py: the same generator, the same seeds, the same order of draws
t0 = time.time()
g = torch.Generator(device=dev).manual_seed(7)
N0, V, R = a.docs, a.terms, 256
lens = torch.exp(np.log(a.mean_len) - 0.32 + 0.8 * torch.randn(N0, generator=g, device=dev)).clamp_(8, 5000).to(torch.int64)
off0 = torch.zeros(N0 + 1, dtype=torch.int64, device=dev)
off0[1:] = torch.cumsum(lens, 0)
T0 = int(off0[-1])
w = 1.0 / torch.arange(1, V, device=dev, dtype=torch.float64) ** 1.07
cdf = (torch.cumsum(w, 0) / w.sum()).to(torch.float32)
tok0 = (torch.searchsorted(cdf, torch.rand(T0, generator=g, device=dev)).clamp_(max=V - 2) + 1).to(torch.int32)
start = off0[:-1]
city = torch.rand(N0, generator=g, device=dev) < 0.85
tok0[start[city]] = 0                                        # the city: first token of 85 % of the documents
rare = V + torch.arange(7 * R, device=dev, dtype=torch.int32).reshape(R, 7)
for r in range(R):
    d = torch.randint(0, N0, (40,), generator=g, device=dev)
    for j in range(2):
        tok0[start[d[:20]] + 2 + j] = rare[r, j]
    for j in range(5):
        tok0[start[d[20:]] + 2 + j] = rare[r, 2 + j]
n_terms = V + 7 * R
# behind the generator's draws: the long document
long_tok = (torch.searchsorted(cdf, torch.rand(a.long_tokens, generator=g, device=dev)).clamp_(max=V - 2) + 1).to(torch.int32)
N = N0 + 1
off = torch.cat([off0, off0[-1:] + a.long_tokens])
tok = torch.cat([tok0, long_tok])
T = int(off[-1])
ix = bm25_index_from_token_ids(np.arange(N, dtype=np.int64), off, tok, n_terms, device=dev, keep_tokens=True)
log(f"corpus {N} docs, {T} tokens, {int(ix.post_doc.numel())} postings in {time.time() - t0:.1f}s")
Q, K, SPAN = a.queries, a.results, a.span
term_off, post_doc = ix.term_off.cpu().numpy(), ix.post_doc.cpu().numpy()
df = np.diff(term_off)
h_off, h_tok = off.cpu().numpy(), tok.cpu().numpy()
h_len = np.diff(h_off)
mid = np.nonzero((df >= 1000) & (df < 10000))[0]
mid = mid[(mid < V) & (mid > 0)]
rng = np.random.default_rng(1)
out = {"docs": N, "tokens": T, "queries": Q, "results": K, "span": SPAN, "iters": a.iters,
       "device": torch.cuda.get_device_name(0)}

eng = DeviceEngine(ix, device=0, max_queries=max(Q, 16), max_k=16, rerank_max_docs=0)
assert eng.has_tokens


def pairs_for(n_row_terms):
    rows, docs = [], []
    for q in range(Q):
        words = rng.choice(mid, n_row_terms - 1, replace=False).tolist()
        rows.append([0] + [int(t) for t in words])
        plist = post_doc[term_off[words[0]]:term_off[words[0] + 1]]
        docs.append(rng.choice(plist, K, replace=len(plist) < K))
    weights = [term_weights(ix, row) for row in rows]
    return rows, weights, np.concatenate(docs).astype(np.int32), np.repeat(np.arange(Q, dtype=np.int32), K)


for L in (3, 8):
    rows, weights, pair_doc, pair_row = pairs_for(L)
    d_doc, d_row = torch.from_numpy(pair_doc).to(dev), torch.from_numpy(pair_row).to(dev)
    res = {"pairs": int(len(pair_doc))}
    # the engine call with the pairs on the device: the lists' one upload and the launch
    res["engine_call_ms"] = timed(lambda: eng.best_windows(d_doc, d_row, rows, weights, SPAN), a.iters)
    got = [x.cpu().numpy() for x in eng.best_windows(d_doc, d_row, rows, weights, SPAN)]
    # the kernel alone: the ABI call on buffers that are already there
    P = lambda t: C.c_void_p(t.data_ptr())
    I32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    r_off = I32(np.concatenate([[0], np.cumsum([len(p) for p in rows])]).tolist())
    r_terms, r_wts, r_span = I32([t for p in rows for t in p]), I32([v for p in weights for v in p]), I32([SPAN] * Q)
    n = len(pair_doc)
    outs = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3)] + \
           [torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int32, device=dev)]

    def kernel(doc=d_doc):
        rc = eng.lib.msr_best_windows(eng.handle, n, P(doc), P(d_row), Q, P(r_off), P(r_terms), P(r_wts), P(r_span),
                                      *[P(t) for t in outs], eng._stream())
        assert rc == 0, rc

    res["kernel_ms"] = timed(kernel, a.iters)
    read = 4 * int(h_len[pair_doc].sum())
    res.update(read_bytes=read, written_bytes=28 * n, windows=int((got[0] >= 0).sum()),
               of_peak=(read + 28 * n) / res["kernel_ms"][0] / 1e6 / PEAK_GBS)
    # one 100 000-token document among the pairs: its wave walks it alone
    long_doc = d_doc.clone()
    long_doc[0] = N - 1
    res["kernel_with_long_document_ms"] = timed(lambda: kernel(long_doc), a.iters)
    res["kernel_again_ms"] = timed(kernel, a.iters)
    # the same answers with numpy on the host
    t = time.perf_counter()
    want = best_windows_fast(h_off, h_tok, pair_doc, pair_row, rows, weights, [SPAN] * Q, n_terms)
    res["host_numpy_ms"] = (time.perf_counter() - t) * 1e3
    same = all(np.array_equal(x.view(y.dtype), y) for x, y in zip(got, want))
    res["equal_to_host"] = bool(same)
    assert same, L
    out[f"rows_of_{L}"] = res
    log(f"rows_of_{L}", json.dumps(res))
eng.close()

if not a.no_batch:
    # ---- Retriever.search_batch with and without snippets: pages, a vocabulary and one chunk vector per document
    def word(t):
        if t == 0:
            return "tübingen"
        s, t = "", int(t)
        while True:
            s = chr(ord("a") + t % 26) + s
            t //= 26
            if t == 0:
                return "w" + s

    class Pages:
        """ix.texts without a million strings: page d is rendered from its token stream on first access and kept."""

        def __init__(self):
            self.kept = {}

        def __len__(self):
            return N

        def __getitem__(self, d):
            page = self.kept.get(d)
            if page is None:
                page = self.kept[d] = " ".join(word(t) for t in h_tok[h_off[d]:h_off[d + 1]].tolist())
            return page

    t0 = time.time()
    ix.vocab = {word(t): t for t in range(n_terms)}
    ix.texts = Pages()
    ix.doc_off = torch.arange(N + 1, dtype=torch.int32)
    ix.chunk_ids = torch.arange(N, dtype=torch.int64)
    emb = torch.randn((N, 768), generator=torch.Generator(device=dev).manual_seed(3), device=dev)
    ix.emb = emb / emb.norm(dim=1, keepdim=True)
    r = Retriever(indexer=DeviceEngine(ix, device=0, max_queries=Q, max_k=1000, rerank_max_docs=1000))
    log(f"retriever in {time.time() - t0:.1f}s")
    queries = [" ".join(word(int(t)) for t in rng.choice(mid, 3, replace=False)) for _ in range(Q)]
    qv = torch.randn((Q, 768), generator=torch.Generator().manual_seed(4)).numpy()
    kw = dict(query_embeddings=qv)
    res = {"search_batch_ms": host_timed(lambda: r.search_batch(queries, **kw), 3),
           "search_batch_snippets_ms": host_timed(lambda: r.search_batch(queries, snippets=True, snippet_tokens=SPAN, **kw), 3)}
    # the snippet step alone, in its three parts
    ids, qvec = r._prepare(queries, qv, None)
    doc, score, _, n = r.final_lists(ids, qvec, 1000)
    rows = [query_row(ix, ids[q]) for q in range(Q)]
    weights = [term_weights(ix, row) for row in rows]
    pq = np.repeat(np.arange(Q), n)
    pr = np.concatenate([np.arange(int(k)) for k in n])
    pair_doc = doc[pq, pr]
    res["pairs"] = int(len(pq))
    res["kernel_call_ms"] = host_timed(lambda: r.engine.best_windows(pair_doc, pq, rows, weights, SPAN), a.iters)
    dev_out = r.engine.best_windows(pair_doc, pq, rows, weights, SPAN)
    res["copies_ms"] = host_timed(lambda: [x.cpu().numpy() for x in dev_out], a.iters)
    s_, _, _, m_, _ = [x.cpu().numpy() for x in dev_out]
    m_ = m_.view(np.uint64)

    def render_all():
        for i in range(len(pq)):
            if s_[i] >= 0:
                render(None, ix.texts[int(pair_doc[i])], int(s_[i]), int(m_[i]), SPAN)

    res["render_ms"] = host_timed(render_all, 3)
    res["windows"] = int((s_ >= 0).sum())
    out["batch"] = res
    log("batch", json.dumps(res))
    r.engine.close()
print(json.dumps(out))
