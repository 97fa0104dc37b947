"""Document side of the encoder (indexer/indexer.py:95-110,157-172): msr_enc_attention_long against the float64
restatement oracle/encoder_ref.py, QueryEncoder.encode_chunks against that restatement and against transformers'
ModernBertModel on the same random weights, and chunk_index.embed_documents -> attach_chunks -> Retriever end to end."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

U32 = 2.0 ** -24                                              # float32 unit roundoff
CLS, SEP = 50281, 50282                                       # ModernBERT's [CLS] / [SEP]


@pytest.fixture(scope="module")
def doc_world():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from transformers import ModernBertConfig, ModernBertModel
    from msretr.encoder import QueryEncoder
    torch.manual_seed(41)
    cfg = ModernBertConfig(reference_compile=False, attn_implementation="eager")
    hf = ModernBertModel(cfg).eval()
    with torch.no_grad():                                     # LayerNorm weights away from 1 so that they matter
        for n, p in hf.named_parameters():
            if n.endswith("norm.weight"):
                p.add_(0.2 * torch.randn_like(p))
    hf = hf.to("cuda")
    enc = QueryEncoder(hf.state_dict(), device=0, use_graphs=False)
    return hf, enc


def _abi(enc):
    import ctypes as C
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    return enc.lib, P, C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _packed(lens):
    """seq_off with empty sequences first, between every two sequences and last."""
    full = [0]
    for n in lens:
        full += [n, 0]
    return np.concatenate([[0], np.cumsum(full)]).astype(np.int32)


def _run_long(enc, qkv, off, n_heads, freqs, window, max_len, guard=2):
    """msr_enc_attention_long on float32 qkv [n_tok][3][n_heads][64] (a device tensor); `guard` rows after the output must
    stay untouched."""
    lib, P, S = _abi(enc)
    n_tok = int(off[-1])
    o = torch.full((n_tok + guard, n_heads * 64), 7.0, device="cuda")
    d_off = torch.from_numpy(np.asarray(off, np.int32)).cuda()
    d_f = torch.as_tensor(np.asarray(freqs, np.float32)).cuda()
    assert lib.msr_enc_attention_long(P(qkv), P(d_off), len(off) - 1, n_heads, P(d_f), window, max_len, P(o), S) == 0
    assert bool((o[n_tok:] == 7.0).all()), "rows past the last token were written"
    return o[:n_tok].double()


def _long_bar(qkv, off):
    """Bar of |kernel - float64| from the float32 arithmetic of msr_enc_attention_long, per
    test_gpu_encoder._attention_bar's derivation, with the two steps the tiled form adds.  A score is a 64-term fmaf
    chain on the matrix cores (16 MFMAs of 4 products) of q and k rotated by the same float32 operations as the short
    kernels: random-walk error 8 u of sum |q_j k_j| / 8 <= |q||k| / 8; a softmax weight then errs by <= 2 max|score
    error| + expf (2 ulp), i.e. 16 u |q||k| / 8 relative.  The S-term sums of weights and of weights x v add sqrt(S) u.
    Online softmax rescales the accumulator and the denominator once per key tile (T = ceil(S / 64) tiles, each a
    float32 product: sqrt(T) u, twice).  So |out error| <= max|v| (16 u max|q||k| / 8 + (sqrt(S) + 2 sqrt(T) + 8) u)."""
    q = qkv.double()
    nq = float(q[:, 0].norm(dim=-1).max())
    nk = float(q[:, 1].norm(dim=-1).max())
    vmax = float(q[:, 2].abs().max())
    smax = int(np.diff(off).max())
    T = -(-smax // 64)
    return vmax * (16 * U32 * nq * nk / 8 + (smax ** 0.5 + 2 * T ** 0.5 + 8) * U32), vmax


LENGTHS = [1, 33, 127, 128, 129, 255, 256, 257, 511, 512, 514, 1000, 2048]


def _seq_rows(off, min_len):
    rows = [np.arange(s, e) for s, e in zip(off[:-1], off[1:]) if e - s >= min_len]
    return torch.from_numpy(np.concatenate(rows)) if rows else torch.zeros(0, dtype=torch.int64)


def test_long_attention_against_float64(doc_world):
    """msr_enc_attention_long against oracle.encoder_ref.attention (float64, on the GPU) at every length of LENGTHS packed
    with empty sequences between them, 3 heads, windows 0 / 3 / 64, both rotary bases, flat (O(0.1)) and peaked (O(10))
    scores; max_len the pack's longest sequence and 0 (no better bound than 8192).  Negative controls on the same data:
    positions that run on across the pack and windows of 63 and 65 must MISS the bar on the sequences of >= 512 tokens.
    Rotary embedding is relative (q.k depends on the difference of the positions), so run-on positions change a score
    only through the float32 rounding of the larger angles: that shows above the bar on peaked scores (|q||k| / 8 ~ 70),
    not on flat ones, and the positions control runs on the peaked data."""
    from oracle import encoder_ref
    _, enc = doc_world
    g = torch.Generator(device="cuda").manual_seed(5)
    off = _packed(LENGTHS)
    n_tok, n_heads = int(off[-1]), 3
    long_rows = _seq_rows(off, 512).cuda()
    worst = {}
    for scale in (0.3, 3.0):                                   # q.k / 8 ~ N(0, scale**4): O(0.1) and O(10)
        qkv = torch.randn((n_tok, 3, n_heads, 64), generator=g, device="cuda") * scale
        bar, vmax = _long_bar(qkv, off)
        for theta in (encoder_ref.THETA_LOCAL, encoder_ref.THETA_GLOBAL):
            freqs = encoder_ref.inv_freq(theta).numpy()
            for window in (64, 0, 3):
                got = _run_long(enc, qkv, off, n_heads, freqs, window, max(LENGTHS))
                want = encoder_ref.attention(qkv, off, n_heads, freqs, window)
                err = float((got - want).abs().max())
                assert err <= bar, (scale, theta, window, err, bar)
                worst[scale] = max(worst.get(scale, (0.0, 0.0)), (err / vmax, bar / vmax))
                if window == 64 and theta == encoder_ref.THETA_LOCAL:
                    assert torch.equal(_run_long(enc, qkv, off, n_heads, freqs, window, 0), got)     # max_len 0
                    for w_bad in (63, 65):
                        bad = encoder_ref.attention(qkv, off, n_heads, freqs, w_bad)
                        e_bad = float((got - bad)[long_rows].abs().max())
                        print(f"  negative control window {w_bad}, scale {scale}: {e_bad / vmax:.3e} (bar {bar / vmax:.3e})")
                        assert e_bad > bar, ("window", w_bad, scale, e_bad, bar)
                if window in (0, 64) and scale == 3.0:
                    bad = encoder_ref.attention(qkv, off, n_heads, freqs, window, run_on_positions=True)
                    e_bad = float((got - bad)[long_rows].abs().max())
                    print(f"  negative control run-on positions, window {window}, theta {theta:g}: {e_bad / vmax:.3e} "
                          f"(bar {bar / vmax:.3e})")
                    assert e_bad > bar, ("run-on positions", window, scale, theta, e_bad, bar)
    for s, (e, b) in worst.items():
        print(f"long attention, scale {s}: max |kernel - float64| / max|v| = {e:.3e} (bar {b:.3e})")


def test_long_attention_8192_tokens_against_float64(doc_world):
    """One sequence of 8192 tokens (ModernBERT's max_position_embeddings) with 1 and 2 heads, global and local layer."""
    from oracle import encoder_ref
    _, enc = doc_world
    g = torch.Generator(device="cuda").manual_seed(8192)
    off = np.array([0, 8192], np.int32)
    for n_heads in (1, 2):
        for scale in (0.3, 3.0):
            qkv = torch.randn((8192, 3, n_heads, 64), generator=g, device="cuda") * scale
            bar, vmax = _long_bar(qkv, off)
            for glob in (True, False):
                freqs = encoder_ref.inv_freq(encoder_ref.THETA_GLOBAL if glob else encoder_ref.THETA_LOCAL).numpy()
                window = 0 if glob else 64
                got = _run_long(enc, qkv, off, n_heads, freqs, window, 8192)
                want = encoder_ref.attention(qkv, off, n_heads, freqs, window)
                err = float((got - want).abs().max())
                print(f"8192 tokens, {n_heads} heads, scale {scale}, global {glob}: max |kernel - float64| / max|v| = "
                      f"{err / vmax:.3e} (bar {bar / vmax:.3e})")
                assert err <= bar, (n_heads, scale, glob, err, bar)


def test_long_attention_window_edge_closed_form(doc_world):
    """inv_freq = 0 and q = 0 make every score exactly 0: the kernel then returns the plain mean of the kept keys' v.  With
    v[k][0] = k (integers below 2**24: exact float32 sums, weights exactly 1) out[t][0] is the float32 division of the
    sum of the kept positions by their count.  Windows 3, 64 and 100 (a window edge inside a key tile, on tiles that
    straddle it) and 0, at lengths up to 2048; bit for bit."""
    _, enc = doc_world
    rng = np.random.default_rng(77)
    lens = [129, 514, 1000, 2048, 65, 1]
    off = _packed(lens)
    n_tok = int(off[-1])
    for n_heads in (1, 3):
        qkv = rng.standard_normal((n_tok, 3, n_heads, 64)).astype(np.float32)
        qkv[:, 0] = 0.0
        pos = np.concatenate([np.arange(e - s) for s, e in zip(off[:-1], off[1:])]).astype(np.int64)
        qkv[:, 2, :, 0] = pos[:, None]
        d_qkv = torch.from_numpy(qkv).cuda()
        for window in (64, 3, 100, 0):
            got = _run_long(enc, d_qkv, off, n_heads, np.zeros(32, np.float32), window, 2048)
            got = got.cpu().numpy().reshape(n_tok, n_heads, 64)[:, :, 0]
            S = np.repeat(np.diff(off), np.diff(off))
            lo = np.maximum(0, pos - window) if window > 0 else np.zeros_like(pos)
            hi = np.minimum(S - 1, pos + window) if window > 0 else S - 1
            cnt = hi - lo + 1
            tot = (lo + hi) * cnt // 2
            want = (tot.astype(np.float32) / cnt.astype(np.float32)).astype(np.float32)
            bad = np.nonzero(~np.all(got == want[:, None], axis=1))[0]
            assert len(bad) == 0, (window, n_heads, bad[:5], got[bad[:5]], want[bad[:5]])


def test_long_attention_nan_contract_and_arguments(doc_world):
    """A sequence longer than max_len gets NaN in all of its rows and the other sequences' rows are bit for bit those of
    a run without it; max_len > 8192, a negative max_len and unaligned buffers are refused."""
    from oracle import encoder_ref
    _, enc = doc_world
    lib, P, S = _abi(enc)
    g = torch.Generator(device="cuda").manual_seed(3)
    freqs = encoder_ref.inv_freq(encoder_ref.THETA_LOCAL).numpy()
    for max_len, too_long in ((650, 700), (64, 65), (0, 8193)):
        lens = [5, too_long, 3, max_len or 600]
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        qkv = torch.randn((int(off[-1]), 3, 12, 64), generator=g, device="cuda")
        got = _run_long(enc, qkv, off, 12, freqs, 64, max_len)
        a, b = int(off[1]), int(off[2])
        assert bool(torch.isnan(got[a:b]).all()), (max_len, too_long)
        keep = torch.cat([torch.arange(0, a), torch.arange(b, int(off[-1]))]).cuda()
        rest = np.concatenate([[0], np.cumsum([lens[0]] + lens[2:])]).astype(np.int32)
        alone = _run_long(enc, qkv[keep].contiguous(), rest, 12, freqs, 64, max_len)
        assert not bool(torch.isnan(alone).any()) and torch.equal(got[keep], alone), (max_len, too_long)
    q = torch.zeros((8, 3, 12, 64), device="cuda")
    o = torch.zeros((9, 768), device="cuda")
    d_off = torch.tensor([0, 8], dtype=torch.int32, device="cuda")
    d_f = torch.as_tensor(freqs).cuda()
    assert lib.msr_enc_attention_long(P(q), P(d_off), 1, 12, P(d_f), 64, 8193, P(o), S) < 0
    assert b"max_len=8193" in lib.msr_last_error(None)
    assert lib.msr_enc_attention_long(P(q), P(d_off), 1, 12, P(d_f), 64, -1, P(o), S) < 0
    assert lib.msr_enc_attention_long(P(q), P(d_off), 1, 12, P(d_f), 64, 8, P(o[0, 1:]), S) < 0     # 4-byte offset
    assert lib.msr_enc_attention_long(P(q), P(d_off), 0, 12, P(d_f), 64, 8, P(o), S) == 0


# ------------------------------------------------------------------ the 22-layer model on document windows
# Bar of max |encode_chunks - float64| over the pooled values.  tests/test_gpu_encoder.py sets E2E_BAR = 3e-6 for
# sequences of <= 128 tokens (2.5 x its measured 1.19e-6).  Of the sums of the forward pass only the attention's grow with
# the sequence (sqrt(514 / 128) ~ 2 x more rounding; the projections' lengths do not change and the mean pool averages
# errors down), so the bar for 514-token windows is twice the query bar.  The same bar holds against transformers'
# float32 model.
DOC_BAR = 6e-6


def _hf_pooled(hf, seqs, pad_id=50283):
    L = max(len(s) for s in seqs)
    ids = torch.full((len(seqs), L), pad_id, dtype=torch.long)
    mask = torch.zeros((len(seqs), L), dtype=torch.long)
    for i, s in enumerate(seqs):
        ids[i, :len(s)] = torch.tensor(s)
        mask[i, :len(s)] = 1
    with torch.no_grad():
        h = hf(input_ids=ids.cuda(), attention_mask=mask.cuda()).last_hidden_state
    m = mask.cuda().unsqueeze(-1).to(h.dtype)
    return (h * m).sum(1) / m.sum(1).clamp(min=1)            # sentence-transformers mean pooling


def _windows(rng, lens):
    return [[CLS] + rng.integers(0, 50000, size=n - 2).tolist() + [SEP] for n in lens]


def test_document_windows_end_to_end(doc_world):
    """encode_chunks (22 layers, normalize off and on) on 514-token windows and shorter ones against
    oracle.encoder_ref.forward in float64 on the GPU and against transformers.ModernBertModel (eager attention, float32)
    + mean pooling on the same weights; two runs bit-identical; other batch splits within the bar."""
    from oracle import encoder_ref
    hf, enc = doc_world
    rng = np.random.default_rng(514)
    seqs = _windows(rng, [514, 514, 514, 200, 3, 514])
    w = {k: v.double() for k, v in hf.state_dict().items()}
    want = encoder_ref.forward(w, seqs, device="cuda")
    got = enc.encode_chunks(seqs, normalize=False).double()
    err = float((got - want).abs().max())
    ref = _hf_pooled(hf, seqs).double()
    err_hf = float((got - ref).abs().max())
    print(f"514-token windows: max |encoder - float64| = {err:.3e}, max |encoder - transformers| = {err_hf:.3e} "
          f"(bar {DOC_BAR:.1e})")
    assert err <= DOC_BAR and err_hf <= DOC_BAR
    again = enc.encode_chunks(seqs, normalize=False).double()
    assert torch.equal(again, got)
    for bt in (514, 1100):                                    # one window per pass; two per pass
        split = enc.encode_chunks(seqs, normalize=False, batch_tokens=bt).double()
        e = float((split - want).abs().max())
        print(f"  batch_tokens {bt}: max |encoder - float64| = {e:.3e}")
        assert e <= DOC_BAR and float((split - got).abs().max()) <= DOC_BAR
    nrm = enc.encode_chunks(seqs)                             # normalize=True: sentence-transformers Normalize
    assert float((nrm.norm(dim=1) - 1).abs().max()) <= 1e-6
    want_n = encoder_ref.forward(w, seqs, device="cuda", normalize=True)
    assert float((nrm.double() - want_n).abs().max()) <= DOC_BAR
    out = torch.full((len(seqs) + 3, 768), 7.0, device="cuda")
    enc.encode_chunks(seqs[:2], out=out, row0=2)              # rows written at their chunk row, nothing else touched
    assert bool((out[:2] == 7.0).all()) and bool((out[4:] == 7.0).all())
    assert float((out[2:4] - nrm[:2]).abs().max()) <= DOC_BAR
    with pytest.raises(ValueError):
        enc.encode_chunks([[1] * 8193])
    enc.max_seq_length = 512                                  # sentence_bert_config.json max_seq_length
    try:
        t = enc.encode_chunks([[1] * 600])
    finally:
        enc.max_seq_length = None
    assert torch.equal(t, enc.encode_chunks([[1] * 512]))


def test_embed_documents_index_and_retriever(doc_world):
    """embed_documents on synthetic token-id documents -> bm25_index_from_token_ids -> attach_chunks ->
    Retriever.quick_search: unit rows; a document's own window as the query finds that document first with cosine
    >= 1 - 1e-5; the dense top-10 equals a float64 brute-force ranking over oracle.encoder_ref embeddings wherever the
    score gaps exceed the bar.  Bar of a cosine: each unit vector errs by <= sqrt(768) DOC_BAR in norm, so a cosine errs by
    <= 2 sqrt(768) DOC_BAR (plus the scan's 1e-5)."""
    from oracle import encoder_ref
    from msretr.chunk_index import attach_chunks, embed_documents
    from msretr.index_build import bm25_index_from_token_ids
    from msretr.retriever import Retriever
    hf, enc = doc_world
    rng = np.random.default_rng(9)
    n_terms = 3000
    lens = [1, 40, 511, 512, 513, 962, 963, 1300, 200, 700, 0, 90]
    doc_ids = rng.permutation(1000)[:len(lens)] + 5
    docs = [(int(d), rng.integers(0, n_terms, size=n).tolist()) for d, n in zip(doc_ids, lens)]
    table = embed_documents(enc, docs, cls_id=CLS, sep_id=SEP)
    assert float((table.emb.norm(dim=1) - 1).abs().max()) <= 1e-6
    tok_off = np.concatenate([[0], np.cumsum([len(t) for _, t in docs])])
    ix = bm25_index_from_token_ids([d for d, _ in docs], tok_off, np.concatenate([t for _, t in docs]).astype(np.int32),
                                   n_terms, device="cuda")
    ix = attach_chunks(ix, table)
    r = Retriever(embedder=enc, indexer=ix)
    w = {k: v.double() for k, v in hf.state_dict().items()}
    want = encoder_ref.forward(w, table.seqs, device="cuda", normalize=True)
    bar = 2 * 768 ** 0.5 * DOC_BAR + 1e-5
    owner = {int(c): int(d) for c, d in zip(table.chunk_ids, table.doc_ids)}
    for probe in (0, 3, len(table) - 1):
        q = enc.encode_chunks([table.seqs[probe]])[0]
        hits = r.quick_search(None, top_k=10, query_embedding=q.cpu().numpy())
        assert hits[0]["doc_id"] == int(table.doc_ids[probe]) and hits[0]["score"] >= 1 - 1e-5, (probe, hits[:2])
        cos = (want @ want[probe]).cpu().numpy()                 # float64 brute force: max over a document's chunks
        best = {}
        for c, s in zip(table.chunk_ids, cos):
            best[owner[int(c)]] = max(best.get(owner[int(c)], -2.0), float(s))
        ranked = sorted(best.items(), key=lambda kv: -kv[1])
        scores = [s for _, s in ranked] + [-2.0]
        for j, h in enumerate(hits):
            lo_gap = scores[j] - scores[j + 1]
            hi_gap = scores[j - 1] - scores[j] if j else 1.0
            if lo_gap > bar and hi_gap > bar:
                assert h["doc_id"] == ranked[j][0], (probe, j, h, ranked[j])
            assert abs(h["score"] - best[h["doc_id"]]) <= bar
