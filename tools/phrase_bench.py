#!/usr/bin/env python3
"""Cost of phrase search (msr_phrase_sets, DeviceEngine.phrase_sets, DESIGN K12): a token-stream corpus built on the GPU with
keep_tokens=True (Zipf ids, planted phrases), 256 rows / queries per mix:
  (a) a rare two-word phrase,  (b) the city + a mid-frequency word,  (c) a five-word phrase,
  (d) one excluded phrase of two frequent words.
Per mix: the device time of the term_sets call that builds the candidate rows, of msr_phrase_sets alone on those rows and of
DeviceEngine.phrase_sets (host packing included) -- events, one warm-up, median of --iters; the byte model (4 bytes per token
of the candidate documents + 4 ceil(N / 32) read and written per row; a hit's early exit is NOT subtracted); and the same
sets built on the host (numpy over the same streams -> pack_within -> upload) on the host clock, asserted equal word for
word.  Prints one JSON line.
    python tools/phrase_bench.py [--docs 1000000] [--rows 256] [--iters 10]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from msretr.docset import DocSet, pack_within  # noqa: E402
from msretr.engine import DeviceEngine  # noqa: E402
from msretr.index_build import bm25_index_from_token_ids  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=1_000_000)
ap.add_argument("--terms", type=int, default=200_000)
ap.add_argument("--mean-len", type=float, default=120.0)
ap.add_argument("--rows", type=int, default=256)
ap.add_argument("--iters", type=int, default=10)
a = ap.parse_args()
dev = torch.device("cuda", 0)
PEAK_GBS = 6100.0                                            # streaming read the README measures (6.1 TB/s)


def log(*x):
    print(*x, file=sys.stderr, flush=True)


def timed(fn, iters):
    """Median device time (ms) of fn() over iters calls, after one warm-up call."""
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
    return float(np.median(ts))


t0 = time.time()
g = torch.Generator(device=dev).manual_seed(7)
N, V, R = a.docs, a.terms, a.rows
lens = torch.exp(np.log(a.mean_len) - 0.32 + 0.8 * torch.randn(N, generator=g, device=dev)).clamp_(8, 5000).to(torch.int64)
off = torch.zeros(N + 1, dtype=torch.int64, device=dev)
off[1:] = torch.cumsum(lens, 0)
T = int(off[-1])
w = 1.0 / torch.arange(1, V, device=dev, dtype=torch.float64) ** 1.07
cdf = (torch.cumsum(w, 0) / w.sum()).to(torch.float32)
tok = (torch.searchsorted(cdf, torch.rand(T, generator=g, device=dev)).clamp_(max=V - 2) + 1).to(torch.int32)
start = off[:-1]
city = torch.rand(N, generator=g, device=dev) < 0.85
tok[start[city]] = 0                                         # the city: first token of 85 % of the documents
# planted phrases: R rare pairs and R five-word runs of otherwise unused ids, each in ~40 documents, at position 2 ..
rare = V + torch.arange(7 * R, device=dev, dtype=torch.int32).reshape(R, 7)
for r in range(R):
    d = torch.randint(0, N, (40,), generator=g, device=dev)
    for j in range(2):
        tok[start[d[:20]] + 2 + j] = rare[r, j]
    for j in range(5):
        tok[start[d[20:]] + 2 + j] = rare[r, 2 + j]
n_terms = V + 7 * R
ix = bm25_index_from_token_ids(np.arange(N, dtype=np.int64), off, tok, n_terms, device=dev, keep_tokens=True)
W = (N + 31) // 32
log(f"corpus {N} docs, {T} tokens, {int(ix.post_doc.numel())} postings in {time.time() - t0:.1f}s")
eng = DeviceEngine(ix, device=0, max_queries=R, max_k=16, rerank_max_docs=0)
assert eng.has_tokens
df = np.diff(ix.term_off.cpu().numpy())
h_off, h_tok = off.cpu().numpy(), tok.cpu().numpy()
h_len = np.diff(h_off)
doc_of = np.repeat(np.arange(N), h_len)
mid = np.nonzero((df >= 1000) & (df < 10000))[0]
mid = mid[mid < V]
freq = np.argsort(-df, kind="stable")[1:33]
rng = np.random.default_rng(1)
pick = rng.permutation(mid)
rare_h = rare.cpu().numpy()
mixes = {   # name -> (phrases, excluded?)
    "a_rare_pair": ([rare_h[r, :2].tolist() for r in range(R)], False),
    "b_city_mid": ([[0, int(pick[r % len(pick)])] for r in range(R)], False),
    "c_five_words": ([rare_h[r, 2:7].tolist() for r in range(R)], False),
    "d_not_frequent_pair": ([[int(freq[r % 32]), int(freq[(r + 1 + r // 32) % 32])] for r in range(R)], True),
}
P = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
I32 = lambda v: torch.tensor(v if len(v) else [0], dtype=torch.int32, device=dev)
out = {"docs": N, "tokens": T, "rows": R, "device": torch.cuda.get_device_name(0)}


def host_mask(p):
    """Documents holding phrase p, numpy over the whole stream (position i + L inside i's document)."""
    L = len(p)
    i = np.nonzero(h_tok[:T - L + 1] == p[0])[0]
    for j in range(1, L):
        i = i[h_tok[i + j] == p[j]]
    i = i[i + L <= h_off[doc_of[i] + 1]]
    m = np.zeros(N, bool)
    m[doc_of[i]] = True
    return m


for name, (phrases, excluded) in mixes.items():
    none = [[] for _ in range(R)]
    cand = eng.term_sets(phrases, None)                      # the candidate rows: the phrase's terms intersected
    term_ms = timed(lambda: eng.term_sets(phrases, None), a.iters)
    p_off = I32(np.concatenate([[0], np.cumsum([len(p) for p in phrases])]).tolist())
    p_terms = I32([t for p in phrases for t in p])
    bits = torch.empty((R, W), dtype=torch.int32, device=dev)

    def call():
        rc = eng.lib.msr_phrase_sets(eng.handle, R, P(p_off), P(p_terms), P(cand.bits), cand.n_sets, cand.stride, P(cand.q_set),
                                     P(bits), W, eng._stream())
        assert rc == 0, rc
    ms = timed(call, a.iters)
    cand_h = cand.bits.cpu().numpy().view(np.uint32)
    rows = cand.q_set.cpu().numpy()
    n_cand, read = 0, 0
    for r in range(R):
        m = np.unpackbits(cand_h[rows[r]].view(np.uint8), bitorder="little")[:N].astype(bool)
        n_cand += int(m.sum())
        read += 4 * int(h_len[m].sum())
    rw = 2 * 4 * W * R
    t = time.perf_counter()
    masks = [host_mask(p) for p in phrases]
    sets = [DocSet(ix, ~m if excluded else m) for m in masks]
    words, q_set, n_sets, stride = pack_within(sets, R, ix)
    host_bits = torch.from_numpy(words.view(np.int32)).to(dev)
    torch.cuda.synchronize()
    host_s = time.perf_counter() - t
    per_q = [[p] for p in phrases]                           # one phrase per query
    facade = (lambda: eng.phrase_sets(None, per_q)) if excluded else (lambda: eng.phrase_sets(per_q))
    ds = facade()
    got = ds.bits[ds.q_set.to(torch.int64)]
    same = bool(torch.equal(host_bits[torch.from_numpy(q_set.astype(np.int64)).to(dev)], got))
    if not excluded:
        same = same and bool(torch.equal(bits, got))
    facade_ms = timed(facade, a.iters)
    out[name] = {"term_sets_ms": term_ms, "phrase_sets_ms": ms, "candidates": n_cand, "matches": int(sum(int(m.sum()) for m in masks)),
                 "read_bytes": read, "bitset_bytes": rw, "model_gbs": (read + rw) / ms / 1e6,
                 "of_peak": (read + rw) / ms / 1e6 / PEAK_GBS, "engine_phrase_sets_ms": facade_ms,
                 "host_route_ms": host_s * 1e3, "equal_to_host_route": same}
    log(name, json.dumps(out[name]))
    assert same, name
eng.close()
print(json.dumps(out))
