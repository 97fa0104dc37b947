#!/usr/bin/env python3
"""Cost of the prefix and wildcard lookup (msr_wildcard_terms, DESIGN K16) on the synthetic vocabulary of tools/fuzzy_bench.py
(10^6 terms, lengths 2 .. 24 around 9, letters a-z and ä ö ü ß with a skewed frequency; weights Zipf-like, 3 % of them 0),
bound to the postings of the corpus tools/phrase_bench.py generates (n_terms = 10^6).  Four mixes of patterns, each cut from
vocabulary terms: `abc*` (a 3-letter prefix), `*xyz` (a 3-letter suffix), `abc*xyz` (head and tail) and `*ab*cd*` (two inner
segments: the general matcher).
  kernel     1, 64 and 256 patterns of a mix, limit 1 and 8 -- the ABI call on buffers that are already there; device events,
             one warm-up, median of --iters with the fastest and the slowest beside it
  filters    what each filter leaves per pattern, counted with numpy over 16 patterns of the mix: after the length tests,
             after the signature, after head and tail (what reaches the general matcher, or, without one, the matches)
  engine     DeviceEngine.wildcard_terms for the same patterns on the host clock: one upload, the two launches, one copy back
  host       the same answers from a compiled `re` over the vocabulary's strings for --host-patterns of the patterns,
             asserted equal to the kernel's
  fuzzy      msr_fuzzy_terms for 256 words (terms with one random edit), tolerance 1 and 2, limit 1: K15 on the same engine
  lexical    msr_bm25_topk for 256 queries of the city and three mid-frequency words, k = 1000, on the same engine
Prints one JSON line.
    python tools/wildcard_bench.py [--terms 1000000] [--docs 1000000] [--iters 10] [--host-patterns 2]"""
import argparse
import ctypes as C
import json
import os
import re
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
ap.add_argument("--host-patterns", type=int, default=2)
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

# ---- the vocabulary of tools/fuzzy_bench.py: V spellings and weights
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
assert eng.lib.msr_bind_vocab(eng.handle, P(keep[0]), P(keep[1]), P(keep[2]), V, len(chars), eng._stream()) == 0
eng._t["voc_off"], eng._t["voc_chars"], eng._t["voc_weight"] = keep       # (what DeviceEngine._bind keeps)
out = {"terms": V, "chars": int(len(chars)), "iters": a.iters, "device": torch.cuda.get_device_name(0)}
LMAX = 32
padded = np.full((V, LMAX), 0xFFFF, np.uint16)
padded[np.arange(LMAX)[None, :] < v_len[:, None]] = chars
right = np.full((V, LMAX), 0xFFFF, np.uint16)                 # right-aligned: the last code point in column 31
right[np.arange(LMAX)[None, :] >= (LMAX - v_len)[:, None]] = chars
spell = lambda t: "".join(chr(c) for c in chars[char_off[t]:char_off[t + 1]])
pool = rng.choice(np.nonzero((v_len >= 8) & (weight > 0))[0], 256, replace=False)


def inner(s):
    i = int(rng.integers(1, len(s) - 5))
    j = int(rng.integers(i + 2, len(s) - 2))
    return "*" + s[i:i + 2] + "*" + s[j:j + 2] + "*"


MIXES = {
    "prefix": [spell(t)[:3] + "*" for t in pool],
    "suffix": ["*" + spell(t)[-3:] for t in pool],
    "head_tail": [spell(t)[:3] + "*" + spell(t)[-3:] for t in pool],
    "inner": [inner(spell(t)) for t in pool],
}


def sig64(codes):
    h = (codes.astype(np.uint64) * np.uint64(0x9E3779B1) & np.uint64(0xFFFFFFFF)) >> np.uint64(26)
    return np.uint64(1) << h


v_sig = np.bitwise_or.reduceat(sig64(chars), char_off[:-1])          # (no term is empty)


def filter_survivors(patterns, sample=16):
    """What the filters leave per pattern, over the first `sample` patterns (these mixes hold no `?`)."""
    n_len = n_sig = n_ht = 0
    for s in patterns[:sample]:
        lits = np.asarray([ord(c) for c in s if c != "*"], np.uint16)
        head, tail = s[:s.index("*")], s[s.rindex("*") + 1:]
        by_len = np.nonzero((weight > 0) & (v_len >= len(lits)))[0]
        n_len += len(by_len)
        sl = np.bitwise_or.reduce(sig64(lits))
        by_sig = by_len[(sl & ~v_sig[by_len]) == 0]
        n_sig += len(by_sig)
        ok = np.ones(len(by_sig), bool)
        for k, c in enumerate(head):
            ok &= padded[by_sig, k] == ord(c)
        for k, c in enumerate(reversed(tail)):
            ok &= right[by_sig, LMAX - 1 - k] == ord(c)
        n_ht += int(ok.sum())
    return {"after_length_tests_per_pattern": n_len / sample, "after_signature_per_pattern": n_sig / sample,
            "after_head_and_tail_per_pattern": n_ht / sample}


words = None


def host_lookup(pattern, limit):
    """A compiled `re` over the vocabulary's strings: every term with a weight, fullmatch."""
    global words
    if words is None:
        words = [spell(t) for t in range(V)]
    rx = re.compile("".join(".*" if c == "*" else "." if c == "?" else re.escape(c) for c in pattern), re.DOTALL)
    ids = np.asarray([t for t in np.nonzero(weight > 0)[0].tolist() if rx.fullmatch(words[t])], np.int64)
    order = np.lexsort((ids, -weight[ids].astype(np.int64)))
    return ids[order][:limit].tolist(), len(ids)


for mix, all_patterns in MIXES.items():
    out[f"filters_{mix}"] = filter_survivors(all_patterns)
    log(f"filters_{mix}", out[f"filters_{mix}"])
    for n_pat in (1, 64, 256):
        pats = all_patterns[:n_pat]
        p_off = np.zeros(n_pat + 1, np.int32)
        np.cumsum([len(s) for s in pats], out=p_off[1:])
        p_chars = np.asarray([ord(c) for s in pats for c in s], np.uint16)
        d_off, d_chars = torch.from_numpy(p_off).to(dev), torch.from_numpy(p_chars.view(np.int16)).to(dev)
        for limit in (1, 8):
            need = int(eng.lib.msr_wildcard_scratch_bytes(V, n_pat, limit))
            scratch = torch.empty((need + 7) // 8, dtype=torch.int64, device=dev)
            outs = [torch.empty(n_pat * limit, dtype=torch.int32, device=dev)] + \
                   [torch.empty(n_pat, dtype=torch.int32, device=dev) for _ in range(2)]

            def kernel():
                rc = eng.lib.msr_wildcard_terms(eng.handle, n_pat, P(d_off), P(d_chars), limit, *[P(t) for t in outs],
                                                P(scratch), need, eng._stream())
                assert rc == 0, eng.lib.msr_last_error(eng.handle)

            res = {"kernel_ms": timed(kernel, a.iters), "scratch_bytes": need,
                   "engine_call_ms": host_timed(lambda: eng.wildcard_terms(pats, limit=limit), a.iters)}
            term, cnt, total = [t.cpu().numpy() for t in outs]
            res["matches_per_pattern"] = float(total.mean())
            if n_pat == 256 and limit == 8:                  # (the host's answers once per mix: each costs most of a second)
                hp = min(a.host_patterns, n_pat)
                t = time.perf_counter()
                want = [host_lookup(s, limit) for s in pats[:hp]]
                res["host_re_ms_per_pattern"] = (time.perf_counter() - t) * 1e3 / hp
                for i, (ids, tot) in enumerate(want):
                    assert term[i * limit:i * limit + int(cnt[i])].tolist() == ids and int(total[i]) == tot, (pats[i], limit)
                res["equal_to_host"] = True
            out[f"{mix}_{n_pat}_limit_{limit}"] = res
            log(f"{mix}_{n_pat}_limit_{limit}", json.dumps(res))


# ---- K15 on the same engine and vocabulary: 256 words with one random edit, tolerance 1 and 2
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
    return s


fz_words = [typo(int(t)) for t in rng.choice(np.nonzero((v_len >= 4) & (weight > 0))[0], 256, replace=False)]
w_off = np.zeros(257, np.int32)
np.cumsum([len(s) for s in fz_words], out=w_off[1:])
w_chars = np.asarray([c for s in fz_words for c in s], np.uint16)
d_off, d_chars = torch.from_numpy(w_off).to(dev), torch.from_numpy(w_chars.view(np.int16)).to(dev)
need = int(eng.lib.msr_fuzzy_scratch_bytes(V, 256, 1))
scratch = torch.empty((need + 7) // 8, dtype=torch.int64, device=dev)
outs = [torch.empty(256, dtype=torch.int32, device=dev) for _ in range(4)]
for m in (1, 2):
    d_max = torch.full((256,), m, dtype=torch.int32, device=dev)

    def fuzzy_kernel():
        rc = eng.lib.msr_fuzzy_terms(eng.handle, 256, P(d_off), P(d_chars), P(d_max), 1, *[P(t) for t in outs], P(scratch), need,
                                     eng._stream())
        assert rc == 0, eng.lib.msr_last_error(eng.handle)

    out[f"fuzzy_256_words_edits_{m}_limit_1_ms"] = timed(fuzzy_kernel, a.iters)
    log(f"fuzzy edits {m}", out[f"fuzzy_256_words_edits_{m}_limit_1_ms"])

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
