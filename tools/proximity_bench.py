#!/usr/bin/env python3
"""Cost of proximity search (msr_proximity_sets, DESIGN K13) beside the exact-phrase kernel it was modelled on: the corpus,
seeds and four mixes of tools/phrase_bench.py (a token-stream corpus built on the GPU with keep_tokens=True; 256 rows per mix):
  (a) a rare two-word phrase,  (b) the city + a mid-frequency word,  (c) a five-word phrase,
  (d) two frequent words (phrase_bench excludes this phrase; the kernels verify it all the same).
Per mix, on the SAME candidate rows (one term_sets call of the rows' terms), back to back in one process -- device events, one
warm-up, median of --iters, with the fastest and the slowest iteration beside it:
  msr_phrase_sets                              the baseline
  msr_proximity_sets ordered, span = L         the same question asked of the ballot scan (asserted equal word for word)
  msr_proximity_sets ordered, span = L + 3
  msr_proximity_sets any order, span = |T| + 8
and the byte model of K12 (4 bytes per token of the candidate documents + 4 ceil(N / 32) read and written per row; a hit's
early exit is NOT subtracted).  For mix (a) the any-order sets are also built on the host (numpy over the same streams ->
pack_within -> upload, host clock) and asserted equal word for word, and DeviceEngine.phrase_sets is timed with Near
conditions (host packing included).  Prints one JSON line.
    python tools/proximity_bench.py [--docs 1000000] [--rows 256] [--iters 10]"""
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
from msretr.text import Near  # noqa: E402

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


# ---- the corpus of tools/phrase_bench.py: the same generator, the same seeds
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
mid = np.nonzero((df >= 1000) & (df < 10000))[0]
mid = mid[mid < V]
freq = np.argsort(-df, kind="stable")[1:33]
rng = np.random.default_rng(1)
pick = rng.permutation(mid)
rare_h = rare.cpu().numpy()
mixes = {
    "a_rare_pair": [rare_h[r, :2].tolist() for r in range(R)],
    "b_city_mid": [[0, int(pick[r % len(pick)])] for r in range(R)],
    "c_five_words": [rare_h[r, 2:7].tolist() for r in range(R)],
    "d_frequent_pair": [[int(freq[r % 32]), int(freq[(r + 1 + r // 32) % 32])] for r in range(R)],
}
P = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
I32 = lambda v: torch.tensor(v if len(v) else [0], dtype=torch.int32, device=dev)
out = {"docs": N, "tokens": T, "rows": R, "iters": a.iters, "device": torch.cuda.get_device_name(0)}


def host_any_order(p, span):
    """Documents that hold every distinct id of p inside a window of `span` tokens, numpy over the whole stream: a match's
    first position holds one of the ids, so every occurrence of an id is tried as the window's start."""
    ids = sorted(set(p))
    at = [np.nonzero(h_tok == t)[0] for t in ids]
    starts = np.unique(np.concatenate(at))
    doc = np.searchsorted(h_off, starts, side="right") - 1
    end = np.zeros(len(starts), np.int64)
    for pos in at:
        k = np.searchsorted(pos, starts)
        end = np.maximum(end, np.where(k < len(pos), pos[np.minimum(k, len(pos) - 1)], T + span))
    ok = (end < h_off[doc + 1]) & (end - starts + 1 <= span)
    m = np.zeros(N, bool)
    m[doc[ok]] = True
    return m


for name, phrases in mixes.items():
    cand = eng.term_sets(phrases, None)                      # the candidate rows: the rows' terms intersected
    p_off = I32(np.concatenate([[0], np.cumsum([len(p) for p in phrases])]).tolist())
    p_terms = I32([t for p in phrases for t in p])
    L = [len(p) for p in phrases]
    variants = {"ordered_span_L": (L, 1), "ordered_span_L3": ([v + 3 for v in L], 1),
                "any_order_span_T8": ([len(set(p)) + 8 for p in phrases], 0)}
    bits = {k: torch.empty((R, W), dtype=torch.int32, device=dev) for k in ("phrase",) + tuple(variants)}
    cand_args = (P(cand.bits), cand.n_sets, cand.stride, P(cand.q_set))

    def phrase_call():
        rc = eng.lib.msr_phrase_sets(eng.handle, R, P(p_off), P(p_terms), *cand_args, P(bits["phrase"]), W, eng._stream())
        assert rc == 0, rc

    def prox_call(key, spans, ordered):
        d_span, d_ord = I32(spans), I32([ordered] * R)

        def call():
            rc = eng.lib.msr_proximity_sets(eng.handle, R, P(p_off), P(p_terms), P(d_span), P(d_ord), *cand_args, P(bits[key]), W,
                                            eng._stream())
            assert rc == 0, rc
        return call

    res = {"phrase_sets_ms": timed(phrase_call, a.iters)}
    for key, (spans, ordered) in variants.items():
        res[key + "_ms"] = timed(prox_call(key, spans, ordered), a.iters)
    res["phrase_sets_again_ms"] = timed(phrase_call, a.iters)           # the baseline once more, behind the others
    cand_h = cand.bits.cpu().numpy().view(np.uint32)
    rows = cand.q_set.cpu().numpy()
    n_cand, read = 0, 0
    for r in range(R):
        m = np.unpackbits(cand_h[rows[r]].view(np.uint8), bitorder="little")[:N].astype(bool)
        n_cand += int(m.sum())
        read += 4 * int(h_len[m].sum())
    rw = 2 * 4 * W * R
    res.update(candidates=n_cand, read_bytes=read, bitset_bytes=rw,
               matches={k: int(np.unpackbits(b.cpu().numpy().view(np.uint8)).sum()) for k, b in bits.items()})
    for k in ("phrase_sets",) + tuple(variants):
        res[k + "_of_peak"] = (read + rw) / res[k + "_ms"][0] / 1e6 / PEAK_GBS
    same = bool(torch.equal(bits["phrase"], bits["ordered_span_L"]))
    res["span_L_equals_phrase_sets"] = same
    assert same, name
    if name == "a_rare_pair":
        spans = variants["any_order_span_T8"][0]
        t = time.perf_counter()
        sets = [DocSet(ix, host_any_order(p, s)) for p, s in zip(phrases, spans)]
        words, q_set, n_sets, stride = pack_within(sets, R, ix)
        host_bits = torch.from_numpy(words.view(np.int32)).to(dev)
        torch.cuda.synchronize()
        res["host_route_ms"] = (time.perf_counter() - t) * 1e3
        per_q = [[Near(p, 8)] for p in phrases]              # one condition per query
        ds = eng.phrase_sets(per_q)
        got = ds.bits[ds.q_set.to(torch.int64)]
        same = bool(torch.equal(host_bits[torch.from_numpy(q_set.astype(np.int64)).to(dev)], got)) and \
            bool(torch.equal(bits["any_order_span_T8"], got))
        res["equal_to_host_route"] = same
        res["engine_phrase_sets_near_ms"] = timed(lambda: eng.phrase_sets(per_q), a.iters)
        assert same, name
    out[name] = res
    log(name, json.dumps(res))
eng.close()
print(json.dumps(out))
