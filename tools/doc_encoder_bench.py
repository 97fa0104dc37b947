#!/usr/bin/env python3
"""Document-side encoder throughput (QueryEncoder.encode_chunks, random ModernBERT-base weights, 22 layers): windows/s for
batches of 514-token windows, msr_enc_attention_long per call for global and local layers at 514 and 2048 tokens, and the
attention's share of the forward pass.  One JSON line.

    python tools/doc_encoder_bench.py [--windows 64] [--tokens 514] [--iters 5]

Times are device events around work that ends in a synchronise, after warm-up.  The attention share is the summed time of
the 22 attention calls of one forward pass (8 global + 14 local, timed alone on the forward pass's own qkv shape) over
the time of that forward pass.  FLOP counts are computed from the shapes (dense attention: 4 S^2 64 per head and
sequence; a local layer counts only the kept keys).
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from msretr import encoder as E  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--windows", type=int, default=64)
ap.add_argument("--tokens", type=int, default=514)
ap.add_argument("--iters", type=int, default=5)
a = ap.parse_args()
assert torch.cuda.is_available(), "doc_encoder_bench.py measures the GPU"

enc = E.QueryEncoder(E.random_weights(seed=0), device=0, use_graphs=False)
rng = np.random.default_rng(1)
P = lambda t: C.c_void_p(t.data_ptr())


def timed(fn, iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters                       # ms


def attention_ms(n_seq, S, glob, iters=20):
    qkv = torch.randn((n_seq * S, 3 * E.HIDDEN), device="cuda")
    out = torch.empty((n_seq * S, E.HIDDEN), device="cuda")
    off = torch.arange(0, (n_seq + 1) * S, S, dtype=torch.int32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    win = 0 if glob else E.LOCAL_WINDOW // 2

    def run():
        rc = enc.lib.msr_enc_attention_long(P(qkv), P(off), n_seq, E.HEADS, P(enc.inv_freq[glob]), win, S, P(out), st)
        assert rc == 0, enc.lib.msr_last_error(None)
    return timed(run, iters)


def attention_flop(n_seq, S, glob):
    w = E.LOCAL_WINDOW // 2
    kept = S * S if glob else sum(min(S - 1, t + w) - max(0, t - w) + 1 for t in range(S))
    return 4.0 * kept * 64 * E.HEADS * n_seq


res = {"windows": a.windows, "tokens_per_window": a.tokens, "layers": enc.layers}
seqs = [rng.integers(0, 50000, size=a.tokens).tolist() for _ in range(a.windows)]
out = torch.empty((a.windows, E.HIDDEN), device="cuda")
fwd = timed(lambda: enc.encode_chunks(seqs, out=out), a.iters)
res["forward_ms"] = round(fwd, 3)
res["windows_per_s"] = round(a.windows / (fwd / 1e3), 1)
n_glob = sum(1 for l in range(enc.layers) if l % E.GLOBAL_EVERY == 0)
n_loc = enc.layers - n_glob
proj_flop = 2.0 * a.windows * a.tokens * enc.layers * (3 * E.HIDDEN * E.HIDDEN + E.HIDDEN * E.HIDDEN
                                                        + 2 * E.INTER * E.HIDDEN + E.INTER * E.HIDDEN)
att_flop = n_glob * attention_flop(a.windows, a.tokens, True) + n_loc * attention_flop(a.windows, a.tokens, False)
res["projection_gflop"] = round(proj_flop / 1e9, 1)
res["attention_gflop"] = round(att_flop / 1e9, 2)
res["forward_tflops"] = round((proj_flop + att_flop) / (fwd / 1e3) / 1e12, 1)
g_ms, l_ms = attention_ms(a.windows, a.tokens, True), attention_ms(a.windows, a.tokens, False)
att_ms = n_glob * g_ms + n_loc * l_ms
res["attention_ms_per_forward"] = round(att_ms, 3)
res["attention_share"] = round(att_ms / fwd, 4)
res["attention_share_target"] = 0.15
for S in (514, 2048):
    n_seq = max(1, a.windows * a.tokens // S)                 # the same token count as the forward pass
    for glob in (True, False):
        ms = attention_ms(n_seq, S, glob)
        key = f"attention_us_{'global' if glob else 'local'}_{n_seq}x{S}"
        res[key] = round(ms * 1e3, 1)
        res[key.replace("_us_", "_tflops_")] = round(attention_flop(n_seq, S, glob) / (ms / 1e3) / 1e12, 1)
print(json.dumps(res))
