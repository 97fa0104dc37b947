#!/usr/bin/env python3
"""Cost of the typo-tolerant lookup (msr_fuzzy_terms, DESIGN K15) on a synthetic vocabulary of 10^6 terms (lengths 2 .. 24
around 9, letters a-z and ä ö ü ß with a skewed frequency, duplicates allowed -- the kernel compares ids, not spellings;
weights Zipf-like, 3 % of them 0), bound to the postings of the corpus tools/phrase_bench.py generates (n_terms = 10^6):
  kernel     1, 64 and 256 words (vocabulary terms with one random edit), tolerance 1 and 2 for every word, limit 1 and 8 --
             the ABI call on buffers that are already there; device events, one warm-up, median of --iters with the fastest
             and the slowest beside it; what the two filters leave per word, counted with numpy over 16 of the words
  engine     DeviceEngine.fuzzy_terms for the same words on the host clock: one upload, the two launches, one copy back
  host       the same answers with numpy on the host for --host-words of the words (the full matrix per term behind a length
             test, vectorised over the terms), asserted equal to the kernel's
  lexical    msr_bm25_topk for 256 queries of the city and three mid-frequency words, k = 1000, on the same engine
Prints one JSON line.
    python tools/fuzzy_bench.py [--terms 1000000] [--docs 1000000] [--iters 10] [--host-words 2]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from msretr.engine import DeviceEngine  # noqa: E402
from msretr.index_build import bm25_index_from_token_ids  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--terms", type=int, default=1_000_000)
ap.add_argument("--docs", type=int, default=1_000_000)
ap.add_argument("--mean-len", type=float, default=120.0)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--host-words", type=int, default=2)
a = ap.parse_args()
dev = torch.device("cuda", 0)


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


# ---- the corpus of tools/phrase_bench.py (the same generator and seeds), over a vocabulary of --terms ids
t0 = time.time()
g = torch.Generator(device=dev).manual_seed(7)
N, V = a.docs, a.terms
lens = torch.exp(np.log(a.mean_len) - 0.32 + 0.8 * torch.randn(N, generator=g, device=dev)).clamp_(8, 5000).to(torch.int64)
off = torch.zeros(N + 1, dtype=torch.int64, device=dev)
off[1:] = torch.cumsum(lens, 0)
T = int(off[-1])
w = 1.0 / torch.arange(1, V, device=dev, dtype=torch.float64) ** 1.07
cdf = (torch.cumsum(w, 0) / w.sum()).to(torch.float32)
tok = (torch.searchsorted(cdf, torch.rand(T, generator=g, device=dev)).clamp_(max=V - 2) + 1).to(torch.int32)
tok[off[:-1][torch.rand(N, generator=g, device=dev) < 0.85]] = 0
ix = bm25_index_from_token_ids(np.arange(N, dtype=np.int64), off, tok, V, device=dev)
del tok
log(f"corpus {N} docs, {T} tokens in {time.time() - t0:.1f}s")

# ---- the vocabulary: V spellings and weights
rng = np.random.default_rng(5)
ALPHA = np.asarray([ord(c) for c in "enisratdhulcgmobwfkzvpäüößjyxq"], np.uint16)
p = 1.0 / np.arange(1, len(ALPHA) + 1) ** 0.9
v_len = np.clip(np.rint(rng.gamma(9.0, 1.05, V)), 2, 24).astype(np.int64)
char_off = np.zeros(V + 1, np.int64)
np.cumsum(v_len, out=char_off[1:])
chars = ALPHA[rng.choice(len(ALPHA), int(char_off[-1]), p=p / p.sum())]
weight = np.maximum(1, (2e6 / (1 + rng.permutation(V)) ** 1.07)).astype(np.uint32)
weight[rng.random(V) < 0.03] = 0
eng = DeviceEngine(ix, device=0, max_queries=256, max_k=1000, rerank_max_docs=0)
keep = (torch.from_numpy(char_off).to(dev), torch.from_numpy(chars.view(np.int16)).to(dev),
        torch.from_numpy(weight.view(np.int32)).to(dev))
P = lambda t: C.c_void_p(t.data_ptr())
owned = eng.owned_bytes()
assert eng.lib.msr_bind_vocab(eng.handle, P(keep[0]), P(keep[1]), P(keep[2]), V, len(chars), eng._stream()) == 0
eng._t["voc_off"], eng._t["voc_chars"], eng._t["voc_weight"] = keep       # (what DeviceEngine._bind keeps: fuzzy_terms works)
out = {"terms": V, "chars": int(len(chars)), "image_bytes": int(char_off.nbytes + chars.nbytes + weight.nbytes),
       "signature_bytes": int(eng.owned_bytes() - owned), "iters": a.iters, "device": torch.cuda.get_device_name(0)}
LMAX = 32
padded = np.full((V, LMAX), 0xFFFF, np.uint16)
padded[np.arange(LMAX)[None, :] < v_len[:, None]] = chars


def typo(t):
    s = chars[char_off[t]:char_off[t + 1]].tolist()
    k, at = int(rng.integers(0, 4)), int(rng.integers(0, len(s)))
    if k == 0:
        s[at] = int(ALPHA[rng.integers(0, len(ALPHA))])
    elif k == 1 and len(s) > 3:
        del s[at]
    elif k == 2:
        s.insert(at, int(ALPHA[rng.integers(0, len(ALPHA))]))
    elif at + 1 < len(s):
        s[at], s[at + 1] = s[at + 1], s[at]
    return "".join(chr(c) for c in s)


pool = np.nonzero((v_len >= 4) & (weight > 0))[0]
all_words = [typo(int(t)) for t in rng.choice(pool, 256, replace=False)]


def sig64(codes):
    h = (codes.astype(np.uint64) * np.uint64(0x9E3779B1) & np.uint64(0xFFFFFFFF)) >> np.uint64(26)
    return np.uint64(1) << h


v_sig = np.bitwise_or.reduceat(sig64(chars), char_off[:-1])          # (no term is empty)
pop = lambda x: np.unpackbits(np.ascontiguousarray(x).view(np.uint8).reshape(-1, 8), axis=1).sum(1)


def filter_survivors(m, sample=16):
    """What the two filters leave per word, over the first `sample` words: the terms that reach the distance."""
    n_len = n_sig = 0
    for s in all_words[:sample]:
        sw = np.bitwise_or.reduce(sig64(np.asarray([ord(c) for c in s], np.uint16)))
        by_len = np.nonzero((weight > 0) & (np.abs(v_len - len(s)) <= m))[0]
        n_len += len(by_len)
        n_sig += int(((pop(sw & ~v_sig[by_len]) <= m) & (pop(v_sig[by_len] & ~sw) <= m)).sum())
    return n_len / sample, n_sig / sample


def host_lookup(word, m, limit):
    """numpy on the host: the length test, then the full matrix of every remaining term, vectorised over the terms."""
    wd = np.asarray([ord(c) for c in word], np.uint16)
    n = len(wd)
    cand = np.nonzero((weight > 0) & (np.abs(v_len - n) <= m))[0]
    sub, L = padded[cand], v_len[cand]
    prev = np.tile(np.arange(n + 1, dtype=np.int32), (len(cand), 1))
    pp, final = None, np.full(len(cand), 99, np.int32)
    for i in range(1, int(L.max(initial=0)) + 1):
        cur = np.empty_like(prev)
        cur[:, 0] = i
        ti = sub[:, i - 1]
        for j in range(1, n + 1):
            c = np.minimum(np.minimum(prev[:, j] + 1, cur[:, j - 1] + 1), prev[:, j - 1] + (ti != wd[j - 1]))
            if i > 1 and j > 1:
                c = np.where((ti == wd[j - 2]) & (sub[:, i - 2] == wd[j - 1]), np.minimum(c, pp[:, j - 2] + 1), c)
            cur[:, j] = c
        final[L == i] = cur[L == i, n]
        pp, prev = prev, cur
    ok = final <= m
    ids, d = cand[ok], final[ok]
    order = np.lexsort((ids, -weight[ids].astype(np.int64), d))
    return ids[order][:limit].tolist(), d[order][:limit].tolist(), int(ok.sum())


for m in (1, 2):
    out[f"filters_edits_{m}"] = dict(zip(("after_length_test_per_word", "after_signature_per_word"), filter_survivors(m)))
    log(f"filters_edits_{m}", out[f"filters_edits_{m}"])
for n_words in (1, 64, 256):
    words = all_words[:n_words]
    w_off = np.zeros(n_words + 1, np.int32)
    np.cumsum([len(s) for s in words], out=w_off[1:])
    w_chars = np.asarray([ord(c) for s in words for c in s], np.uint16)
    d_off, d_chars = torch.from_numpy(w_off).to(dev), torch.from_numpy(w_chars.view(np.int16)).to(dev)
    for m in (1, 2):
        d_max = torch.full((n_words,), m, dtype=torch.int32, device=dev)
        for limit in (1, 8):
            need = int(eng.lib.msr_fuzzy_scratch_bytes(V, n_words, limit))
            scratch = torch.empty((need + 7) // 8, dtype=torch.int64, device=dev)
            outs = [torch.empty(n_words * limit, dtype=torch.int32, device=dev) for _ in range(2)] + \
                   [torch.empty(n_words, dtype=torch.int32, device=dev) for _ in range(2)]

            def kernel():
                rc = eng.lib.msr_fuzzy_terms(eng.handle, n_words, P(d_off), P(d_chars), P(d_max), limit, *[P(t) for t in outs],
                                             P(scratch), need, eng._stream())
                assert rc == 0, eng.lib.msr_last_error(eng.handle)

            res = {"kernel_ms": timed(kernel, a.iters), "scratch_bytes": need,
                   "engine_call_ms": host_timed(lambda: eng.fuzzy_terms(words, max_edits=m, limit=limit), a.iters)}
            term, dist, cnt, total = [t.cpu().numpy() for t in outs]
            res["candidates_per_word"] = float(total.mean())
            res["words_with_a_candidate"] = int((total > 0).sum())
            hw = min(a.host_words, n_words)
            t = time.perf_counter()
            want = [host_lookup(s, m, limit) for s in words[:hw]]
            res["host_numpy_ms_per_word"] = (time.perf_counter() - t) * 1e3 / hw
            for i, (ids, d, tot) in enumerate(want):
                assert term[i * limit:i * limit + int(cnt[i])].tolist() == ids and int(total[i]) == tot, (words[i], m, limit)
                assert dist[i * limit:i * limit + int(cnt[i])].tolist() == d
            res["equal_to_host"] = True
            out[f"words_{n_words}_edits_{m}_limit_{limit}"] = res
            log(f"words_{n_words}_edits_{m}_limit_{limit}", json.dumps(res))

# ---- the lexical stage of a 256-query chunk on the same engine
df = np.diff(ix.term_off.cpu().numpy())
mid = np.nonzero((df >= 1000) & (df < 10000))[0]
mid = mid[mid > 0]
queries = [[0] + [int(t) for t in rng.choice(mid, 3, replace=False)] for _ in range(256)]
packed = eng.pack_queries(queries)
out["lexical_256_queries_ms"] = timed(lambda: eng.bm25_topk(None, k=1000, packed=packed), a.iters)
log("lexical", out["lexical_256_queries_ms"])
eng.close()
print(json.dumps(out))
