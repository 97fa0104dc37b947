"""Query encoder on the GPU against transformers' ModernBertModel -- the reference's own dependency
(sentence-transformers 5.0.0, requirements.txt:13; reranker_api.py:137-139,355) -- on the SAME random weights: the served
checkpoint is fetched by name in the reference and is not available offline, so the architecture is pinned, the trained
weights are not ("parity unpinned" for them).  Container: transformers 5.15.0."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def enc_world():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from transformers import ModernBertConfig, ModernBertModel
    from msretr.encoder import QueryEncoder
    torch.manual_seed(11)
    cfg = ModernBertConfig(reference_compile=False, attn_implementation="eager")
    hf = ModernBertModel(cfg).eval()
    with torch.no_grad():                                     # LayerNorm weights away from 1 so that they matter
        for n, p in hf.named_parameters():
            if n.endswith("norm.weight"):
                p.add_(0.2 * torch.randn_like(p))
    hf = hf.to("cuda")
    enc = QueryEncoder(hf.state_dict(), device=0)
    return hf, enc


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


def test_encoder_matches_transformers_modernbert(enc_world):
    hf, enc = enc_world
    rng = np.random.default_rng(3)
    seqs = [rng.integers(0, 50000, size=n).tolist() for n in (1, 2, 5, 17, 64, 65, 100, 128, 9, 9)]
    got = enc.encode(seqs)
    ref = _hf_pooled(hf, seqs)
    err = float((got - ref).abs().max())
    print(f"max |encoder - transformers| over {len(seqs)} x 768 pooled values: {err:.3e}")
    assert got.shape == (len(seqs), 768) and err <= 3e-6               # measured on the MI355X: 1.43e-6
    # cosine between the two embeddings of every sequence: what the retriever consumes
    cos = torch.nn.functional.cosine_similarity(got, ref, dim=1)
    assert float(cos.min()) > 1 - 1e-6
    # the batch above (400 tokens) runs msr_enc_linear's batch form (64 x 48 tiles); single queries its token-tile forms: one
    # per tile shape of that kernel (1, 17, 65, 128 tokens), same bar against transformers
    for i in (0, 3, 5, 7):
        single = enc.encode([seqs[i]])[0]
        e1 = float((single - ref[i]).abs().max())
        print(f"  {len(seqs[i])} tokens alone: max |encoder - transformers| = {e1:.3e}")
        assert e1 <= 3e-6 and float(torch.nn.functional.cosine_similarity(single, ref[i], dim=0)) > 1 - 1e-6
    # batching does not change a sequence's embedding (no padding token takes part in any product)
    one = enc.encode([seqs[4]])
    assert float((one[0] - got[4]).abs().max()) <= 1e-5
    # replaying the captured hipGraph == launching the kernels one by one, bit for bit; and a second call replays
    enc.use_graphs = False
    eager = enc.encode(seqs)
    enc.use_graphs = True
    assert torch.equal(eager, got) and torch.equal(enc.encode(seqs), got) and len(enc._graphs) >= 1
    nrm = enc.encode(seqs[:3], normalize=True)
    assert torch.allclose(nrm.norm(dim=1), torch.ones(3, device=nrm.device), atol=1e-5)
    assert torch.allclose(nrm, torch.nn.functional.normalize(got[:3], dim=1), atol=1e-6)


def test_encoder_kernels_against_torch_ops(enc_world):
    import ctypes as C
    _, enc = enc_world
    lib, dev = enc.lib, enc.device
    P = lambda t: C.c_void_p(t.data_ptr())
    S = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator(device="cpu"); g.manual_seed(5)
    x = (torch.randn(37, 768, generator=g) * 3 + 0.5).to(dev)
    w = (1 + 0.3 * torch.randn(768, generator=g)).to(dev)
    y = torch.empty_like(x)
    assert lib.msr_enc_layernorm(P(x), None, None, P(w), P(y), 37, 768, C.c_float(1e-5), S) == 0
    assert float((y - torch.nn.functional.layer_norm(x, (768,), w, None, 1e-5)).abs().max()) <= 2e-6
    u = torch.randn(37, 2304, generator=g).to(dev) * 2
    a = torch.empty(37, 1152, device=dev)
    assert lib.msr_enc_geglu(P(u), P(a), 37, 1152, S) == 0
    assert float((a - torch.nn.functional.gelu(u[:, :1152]) * u[:, 1152:]).abs().max()) <= 2e-6
    off = torch.tensor([0, 5, 5, 37], dtype=torch.int32, device=dev)          # an empty sequence in the middle
    out = torch.empty(3, 768, device=dev)
    assert lib.msr_enc_mean_pool(P(x), P(off), 3, 768, 0, P(out), S) == 0
    assert float((out[0] - x[:5].mean(0)).abs().max()) <= 2e-6 and float(out[1].abs().max()) == 0.0
    assert float((out[2] - x[5:].mean(0)).abs().max()) <= 2e-6
    assert lib.msr_enc_layernorm(P(x), None, None, P(w), P(y), 37, 100, C.c_float(1e-5), S) < 0    # unsupported width
    assert b"dim=100" in lib.msr_last_error(None)


def test_encoder_linear_against_float64(enc_world):
    """msr_enc_linear (the skinny matrix product of every projection) against a float64 product: all four shapes of a
    layer, token counts on both sides of every tile size, residual in place, rows past the end untouched."""
    import ctypes as C
    _, enc = enc_world
    lib, dev = enc.lib, enc.device
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    S = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator(device="cpu"); g.manual_seed(23)
    for n_out, n_in in ((2304, 768), (768, 768), (768, 1152)):
        w = (torch.randn(n_out, n_in, generator=g) * 0.05).to(dev)
        for n_tok in (1, 5, 16, 17, 33, 64, 100, 128, 129, 300):
            x = torch.randn(n_tok, n_in, generator=g).to(dev)
            r = torch.randn(n_tok, n_out, generator=g).to(dev)
            want = x.double() @ w.double().t()
            y = torch.full((n_tok + 3, n_out), 7.0, device=dev)                    # 3 guard rows
            assert lib.msr_enc_linear(P(x), P(w), None, P(y), n_tok, n_out, n_in, S) == 0
            scale = float(want.abs().max())
            assert float((y[:n_tok].double() - want).abs().max()) <= 2e-6 * scale, (n_out, n_in, n_tok)
            assert bool((y[n_tok:] == 7.0).all())
            h = r.clone()
            assert lib.msr_enc_linear(P(x), P(w), P(h), P(h), n_tok, n_out, n_in, S) == 0     # h += x . w^T
            assert float((h.double() - (want + r.double())).abs().max()) <= 2e-6 * scale
            again = r.clone()
            assert lib.msr_enc_linear(P(x), P(w), P(again), P(again), n_tok, n_out, n_in, S) == 0
            assert torch.equal(h, again)                                           # fixed summation order
    x = torch.randn(4, 768, generator=g).to(dev); w = torch.randn(48, 768, generator=g).to(dev); y = torch.empty(4, 48, device=dev)
    assert lib.msr_enc_linear(P(x), P(w), None, P(y), 4, 48, 768, S) < 0 and b"n_out=48" in lib.msr_last_error(None)
    assert lib.msr_enc_linear(P(x), P(w), None, P(y), 4, 32, 100, S) < 0
    assert lib.msr_enc_linear(P(x), P(w), None, P(y), 0, 32, 768, S) == 0


def test_encoder_rejects_what_it_cannot_do(enc_world):
    _, enc = enc_world
    with pytest.raises(ValueError):
        enc.encode([[1] * 129])
    with pytest.raises(ValueError):
        enc.encode([[60000]])
    with pytest.raises(ValueError):
        enc.encode(["a query string"])                       # no tokenizer.json was loaded
    assert enc.encode([]).shape == (0, 768) and float(enc.encode([[]]).abs().max()) == 0.0


def test_encoder_from_local_directory_and_in_the_retriever(tmp_path):
    """from_dir: model.safetensors + tokenizer.json + modules.json of a local sentence-transformers directory (a 2-layer
    model and a word-level tokenizer written by this test), then the query STRING path of the host classes
    (reranker_api.py:355 -> Retriever.quick_search) with the encoder as the embedder."""
    from safetensors.torch import save_file
    from tokenizers import Tokenizer, models, pre_tokenizers
    from msretr.encoder import QueryEncoder, random_weights
    from msretr.retriever import Retriever
    from msretr.synthetic import synthetic_corpus
    d = tmp_path / "model"
    d.mkdir()
    w = random_weights(seed=4, layers=2)
    save_file({("model." + k): v.contiguous() for k, v in w.items()}, str(d / "model.safetensors"))
    vocab = {"[UNK]": 0, "tübingen": 1, "castle": 2, "food": 3, "and": 4, "drinks": 5}
    tok = Tokenizer(models.WordLevel(vocab, unk_token="[UNK]"))
    tok.pre_tokenizer = pre_tokenizers.Whitespace()
    tok.save(str(d / "tokenizer.json"))
    (d / "modules.json").write_text('[{"idx": 0, "type": "sentence_transformers.models.Transformer"}, '
                                    '{"idx": 1, "type": "sentence_transformers.models.Pooling"}, '
                                    '{"idx": 2, "type": "sentence_transformers.models.Normalize"}]')
    enc = QueryEncoder.from_dir(str(d), device=0)
    assert enc.layers == 2 and enc.normalize is True
    v = enc.encode("food and drinks")
    assert isinstance(v, np.ndarray) and v.shape == (768,) and abs(float(np.linalg.norm(v)) - 1.0) < 1e-5
    same = enc.encode([[3, 4, 5]], convert_to_numpy=True)[0]
    assert np.array_equal(v, same)                              # the string went through tokenizer.json
    assert not np.allclose(v, enc.encode("tübingen castle"))
    ix = synthetic_corpus(2000, n_chunks=8000, n_terms=1000, device="cuda")
    ix.urls = [f"https://example.org/{i}" for i in range(ix.n_docs)]
    ix.titles = [f"title {i}" for i in range(ix.n_docs)]
    ix.texts = [f"text {i}" for i in range(ix.n_docs)]
    r = Retriever(embedder=enc, indexer=ix)
    hits = r.quick_search("food and drinks", top_k=5, return_unique_docs=True)
    again = r.quick_search(None, top_k=5, query_embedding=v)
    assert len(hits) == 5 and [h["doc_id"] for h in hits] == [h["doc_id"] for h in again]
    with pytest.raises(FileNotFoundError):
        QueryEncoder.from_dir(str(tmp_path))


# ------------------------------------------------------------------ the kernels against oracle/encoder_ref.py (float64)
U32 = 2.0 ** -24                                              # float32 unit roundoff
CLASS_LENGTHS = {8: [1, 7, 8], 16: [9, 15, 16, 1], 32: [17, 31, 32, 9], 0: [33, 64, 65, 66, 127, 128, 1, 8],
                 128: [33, 64, 65, 66, 127, 128, 17]}          # max_len -> lengths; each in the smallest class taking it
CLASS_BOUND = {8: 8, 16: 16, 32: 32, 0: 128, 128: 128}


def _abi(enc):
    import ctypes as C
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    return enc.lib, P, C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _packed(lens, empties=True):
    """seq_off of the lengths with empty sequences first, in the middle and last (an odd count of sequences)."""
    lens = list(lens)
    if empties:
        lens = [0] + lens[: len(lens) // 2] + [0] + lens[len(lens) // 2:] + [0]
    if len(lens) % 2 == 0:
        lens.append(0)
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def _run_attention(enc, qkv, off, n_heads, freqs, window, max_len, guard=2):
    """msr_enc_attention on float32 qkv [n_tok][3][n_heads][64]; `guard` rows after the output must stay untouched."""
    lib, P, S = _abi(enc)
    n_tok = int(off[-1])
    q = torch.from_numpy(np.ascontiguousarray(qkv, np.float32)).cuda()
    o = torch.full((n_tok + guard, n_heads * 64), 7.0, device="cuda")
    d_off = torch.from_numpy(off).cuda()
    d_f = torch.from_numpy(np.asarray(freqs, np.float32)).cuda()
    assert lib.msr_enc_attention(P(q), P(d_off), len(off) - 1, n_heads, P(d_f), window, max_len, P(o), S) == 0
    o = o.cpu()
    assert bool((o[n_tok:] == 7.0).all()), "rows past the last token were written"
    return o[:n_tok].double()


def _attention_bar(qkv, off):
    """Bar of |kernel - float64| over a batch, from the float32 arithmetic of the kernels.  A score is a 64-term float32
    dot product of rotated q and k (rotation: a few roundings per element, cosf / sinf ~2 ulp); its rounding errors add
    up like a random walk, sqrt(64) u = 8 u of sum |q_j k_j| / 8 <= |q||k| / 8 (Cauchy-Schwarz), where the worst case
    would be 64 u.  A softmax weight then errs by <= 2 max|score error| + expf (2 ulp) relative, and the S-term sums of
    weights and of weights x v add sqrt(S) u; so |out error| <= max|v| (16 u max|q||k| / 8 + (sqrt(S) + 8) u).
    Measured on the MI355X (all classes, 1 / 3 / 12 heads, windows 0 / 3 / 64, both bases): scores O(0.1) <= 8.3e-8 max|v|
    (bar >= 1.7e-6), scores O(10) <= 3.6e-6 max|v| (bar >= 1.0e-4)."""
    n_tok = qkv.shape[0]
    nq = np.linalg.norm(qkv[:, 0].astype(np.float64), axis=-1).max()
    nk = np.linalg.norm(qkv[:, 1].astype(np.float64), axis=-1).max()
    smax = int(np.diff(off).max())
    return float(np.abs(qkv[:, 2]).max()) * (16 * U32 * nq * nk / 8 + (smax ** 0.5 + 8) * U32), float(np.abs(qkv[:, 2]).max())


@pytest.mark.parametrize("max_len", [8, 16, 32, 0, 128])
def test_attention_kernels_against_float64(enc_world, max_len):
    """msr_enc_attention against oracle.encoder_ref.attention in every length class, on both sides of every class
    boundary, with empty sequences first / in the middle / last, an odd number of sequences and 1, 3 or 12 heads (so that
    the short kernels' grids end in idle waves), the local window (64), no window (0) and a window of 3 (the only way to
    reach the mask inside the short kernels), both rotary bases, and scores of O(0.1) (flat softmax) and O(10) (peaked)."""
    from oracle import encoder_ref
    rng = np.random.default_rng(100 + max_len)
    off = _packed(CLASS_LENGTHS[max_len])
    n_tok = int(off[-1])
    worst = {}
    for n_heads in (12, 1, 3):
        for scale in (0.3, 3.0):                              # q.k / 8 ~ N(0, scale**4): O(0.1) and O(10)
            qkv = (rng.standard_normal((n_tok, 3, n_heads, 64)) * scale).astype(np.float32)
            bar, vmax = _attention_bar(qkv, off)
            for theta in (encoder_ref.THETA_LOCAL, encoder_ref.THETA_GLOBAL):
                freqs = encoder_ref.inv_freq(theta).numpy()
                for window in (64, 0, 3):
                    got = _run_attention(enc_world[1], qkv, off, n_heads, freqs, window, max_len)
                    want = encoder_ref.attention(qkv, off, n_heads, freqs, window)
                    err = float((got - want).abs().max())
                    assert err <= bar, (max_len, n_heads, scale, theta, window, err, bar)
                    worst[scale] = max(worst.get(scale, (0.0, 0.0)), (err / vmax, bar / vmax))
    for s, (e, b) in worst.items():
        print(f"max_len {max_len}: scale {s}: max |kernel - float64| / max|v| = {e:.3e} (bar {b:.3e})")


def test_attention_bench_shape_against_float64(enc_world):
    """The configuration the bench times: 256 sequences x 8 tokens x 12 heads (3072 pairs of short_kernel<8>)."""
    from oracle import encoder_ref
    rng = np.random.default_rng(256)
    off = np.arange(0, 257 * 8, 8, dtype=np.int32)
    for scale in (0.3, 3.0):
        qkv = (rng.standard_normal((256 * 8, 3, 12, 64)) * scale).astype(np.float32)
        bar, vmax = _attention_bar(qkv, off)
        for glob in (True, False):
            freqs = encoder_ref.inv_freq(encoder_ref.THETA_GLOBAL if glob else encoder_ref.THETA_LOCAL).numpy()
            window = 0 if glob else 64
            got = _run_attention(enc_world[1], qkv, off, 12, freqs, window, 8)
            want = encoder_ref.attention(qkv, off, 12, freqs, window)
            err = float((got - want).abs().max())
            print(f"256 x 8 x 12, scale {scale}, global {glob}: max |kernel - float64| / max|v| = {err / vmax:.3e} "
                  f"(bar {bar / vmax:.3e})")
            assert err <= bar
            # positions restart in every sequence: each sequence alone gives the same rows (same kernel, same arithmetic)
            one = _run_attention(enc_world[1], qkv[8 * 200: 8 * 201], np.array([0, 8], np.int32), 12, freqs, window, 8)
            assert torch.equal(one, got[8 * 200: 8 * 201])


@pytest.mark.parametrize("max_len", [8, 16, 32, 0, 128])
def test_attention_window_edge_closed_form_every_class(enc_world, max_len):
    """inv_freq = 0 and q = 0 make every score exactly 0: each kernel then returns the plain mean of the kept keys' v.
    With v[k][0] = k (integers: exact float32 sums) out[t][0] is the float32 division of the sum of the kept positions
    by their count -- the mean of the k with |k - t| <= window.  A window edge off by one moves it by >= 1/130."""
    rng = np.random.default_rng(7 + max_len)
    bound = CLASS_BOUND[max_len]
    lens = sorted({min(bound, n) for n in (bound, 66, bound - 1, 1, 5)})
    off = _packed(lens)
    n_tok = int(off[-1])
    for n_heads in (1, 3):
        qkv = rng.standard_normal((n_tok, 3, n_heads, 64)).astype(np.float32)
        qkv[:, 0] = 0.0
        pos = np.concatenate([np.arange(e - s) for s, e in zip(off[:-1], off[1:])]).astype(np.float32)
        qkv[:, 2, :, 0] = pos[:, None]
        for window in (64, 3, 0):
            got = _run_attention(enc_world[1], qkv, off, n_heads, np.zeros(32, np.float32), window, max_len)
            got = got.numpy().reshape(n_tok, n_heads, 64)[:, :, 0]
            for s, e in zip(off[:-1], off[1:]):
                for t in range(e - s):
                    ks = [k for k in range(e - s) if window <= 0 or abs(k - t) <= window]
                    want = np.float32(np.float32(sum(ks)) / np.float32(len(ks)))
                    assert np.all(got[s + t] == want), (max_len, window, e - s, t, got[s + t], want)


@pytest.mark.parametrize("max_len", [8, 16, 32, 0, 128])
def test_attention_longer_than_its_class_gets_nan_rows(enc_world, max_len):
    """A sequence longer than its kernel's bound (8 / 16 / 32, or 128 for max_len 0 and 33..128) gets NaN in all of its
    rows, reads nothing past the bound, and the other sequences' rows are bit for bit those of a run without it."""
    from oracle import encoder_ref
    rng = np.random.default_rng(300 + max_len)
    bound = CLASS_BOUND[max_len]
    freqs = encoder_ref.inv_freq(encoder_ref.THETA_LOCAL).numpy()
    for too_long in sorted({bound + 1, 200}):
        lens = [min(5, bound), too_long, 3, bound]
        n = sum(lens)
        qkv = rng.standard_normal((n, 3, 12, 64)).astype(np.float32)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        got = _run_attention(enc_world[1], qkv, off, 12, freqs, 64, max_len)
        a, b = int(off[1]), int(off[2])
        assert bool(torch.isnan(got[a:b]).all()), (max_len, too_long)
        keep = np.r_[0:a, b:n]
        rest = np.concatenate([[0], np.cumsum([lens[0]] + lens[2:])]).astype(np.int32)
        alone = _run_attention(enc_world[1], qkv[keep], rest, 12, freqs, 64, max_len)
        assert torch.equal(got[keep], alone), (max_len, too_long)


def test_layernorm_lookup_dim_1024_against_float64(enc_world):
    """msr_enc_layernorm through the fused lookup (x == NULL, ids / table) at dim 1024 (the PER = 16 instantiation), row
    counts on both sides of the 4 rows of a workgroup, ordinary rows and rows of mean 1e3 / std 1e-2.  Bar per row, from
    the one-pass float32 mean and variance (a lane sums 16 values, then 6 shuffle levels: 22 roundings): the mean errs by
    <= 22 u mean|x|, which moves y by that / std; the variance's 22 roundings move it by <= 11 u |y|; w, the product and
    1/sqrt add 4 u |y|: |error| <= max|w| (22 u mean|x| / std + 16 u max|y / w|).  Measured on the MI355X: 0.10 of the
    bar on ordinary rows, 0.06 of it on the rows of mean 1e3."""
    import ctypes as C
    from oracle import encoder_ref
    lib, P, S = _abi(enc_world[1])
    g = torch.Generator().manual_seed(31)
    vocab = 2000
    table = torch.randn(vocab, 1024, generator=g, dtype=torch.float64) * 2 + 0.3
    table[1000:] = 1e3 + 1e-2 * torch.randn(vocab - 1000, 1024, generator=g, dtype=torch.float64)
    table = table.float()
    w = (1 + 0.3 * torch.randn(1024, generator=g)).float()
    dt, dw = table.cuda(), w.cuda()
    worst = {}
    for n_rows in (1, 3, 4, 5, 1023):
        for lo in (0, 1000):
            ids = torch.randint(lo, lo + 1000, (n_rows,), generator=g, dtype=torch.int32)
            d_ids = ids.cuda()
            y = torch.full((n_rows + 4, 1024), 7.0, device="cuda")
            assert lib.msr_enc_layernorm(None, P(d_ids), P(dt), P(dw), P(y), n_rows, 1024, C.c_float(1e-5), S) == 0
            y = y.cpu()
            assert bool((y[n_rows:] == 7.0).all())
            want = encoder_ref.layernorm_lookup(ids, table, w)
            x = table[ids.long()].double()
            std = x.std(1, unbiased=False)
            bar = float(w.abs().max()) * (22 * U32 * x.abs().mean(1) / std + 16 * U32 * (want / w.double()).abs().amax(1))
            err = (y[:n_rows].double() - want).abs().amax(1)
            assert bool((err <= bar).all()), (n_rows, lo, float(err.max()), float(bar.min()))
            worst[lo] = max(worst.get(lo, 0.0), float((err / bar).max()))
    print(f"layernorm dim 1024 via lookup: max |error| / bar = {worst[0]:.3f} (ordinary rows), {worst[1000]:.3f} "
          f"(mean 1e3, std 1e-2)")


def test_geglu_against_float64_where_erf_saturates(enc_world):
    """msr_enc_geglu on a in [-12, 12] (erf saturates to +-1 beyond ~4), with +-0, against float64.  Bar per element:
    erff's few ulp of absolute error near erf = -1 are a large relative error of 1 + erf, so the bar is absolute in
    |a g|: |error| <= 8 u |a| |g|.  Measured on the MI355X: 2.0 u |a| |g|."""
    from oracle import encoder_ref
    lib, P, S = _abi(enc_world[1])
    half, n_rows = 1152, 3
    a = np.concatenate([np.linspace(-12, 12, half * n_rows - 2), [0.0, -0.0]]).reshape(n_rows, half)
    g = np.random.default_rng(5).standard_normal((n_rows, half)) * 3
    u = np.concatenate([a, g], 1).astype(np.float32)
    y = torch.empty(n_rows, half, device="cuda")
    du = torch.from_numpy(u).cuda()
    assert lib.msr_enc_geglu(P(du), P(y), n_rows, half, S) == 0
    y = y.cpu().double()
    want = encoder_ref.geglu(u)
    bar = 8 * U32 * torch.from_numpy(np.abs(u[:, :half].astype(np.float64) * u[:, half:]))
    err = (y - want).abs()
    print(f"geglu: max |error| / (u |a g|) = {float((err / (bar / 8 + 1e-300)).max()):.2f}")
    assert bool((err <= bar).all())
    assert float(y[-1, -1]) == 0.0 and float(y[-1, -2]) == 0.0 and not bool(torch.isnan(y).any())


def test_mean_pool_normalized_against_float64(enc_world):
    """msr_enc_mean_pool with normalize = 1: a zero vector and an empty sequence give exactly 0 (not NaN); the others are
    unit vectors within (sqrt(S) + 10) u of float64 (S-term float32 sums, then the norm).  Measured on the MI355X: 4.0e-8
    (0.7 u)."""
    from oracle import encoder_ref
    lib, P, S = _abi(enc_world[1])
    g = torch.Generator().manual_seed(9)
    lens = [0, 5, 3, 1, 128, 0, 40]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    h = torch.randn(int(off[-1]), 768, generator=g) * 2 + 0.1
    h[5:8] = 0.0                                              # sequence 2: a zero vector
    out = torch.full((len(lens) + 1, 768), 7.0, device="cuda")
    d_h, d_off = h.cuda(), torch.from_numpy(off).cuda()
    assert lib.msr_enc_mean_pool(P(d_h), P(d_off), len(lens), 768, 1, P(out), S) == 0
    out = out.cpu()
    assert bool((out[-1] == 7.0).all())
    out = out[:-1].double()
    want = encoder_ref.mean_pool(h, off, normalize=True)
    assert not bool(torch.isnan(out).any())
    for b in (0, 2, 5):
        assert bool((out[b] == 0).all()), b
    err = float((out - want).abs().max())
    print(f"mean_pool normalize: max |error| = {err:.3e}")
    assert err <= (max(lens) ** 0.5 + 10) * U32


# ------------------------------------------------------------------ the whole encoder against the 22-layer float64 model
@pytest.fixture(scope="module")
def f64_world(enc_world):
    """oracle.encoder_ref.forward (torch float64 on the GPU) on the fixture's weights, once per module, for the cases of
    the end-to-end tests below."""
    from oracle import encoder_ref
    hf, enc = enc_world
    w = {k: v.double() for k, v in hf.state_dict().items()}
    rng = np.random.default_rng(17)
    cases = {f"single {n}": [rng.integers(0, 50000, size=n).tolist()] for n in (1, 8, 9, 16, 17, 32, 33, 128)}
    cases["256 x 8"] = [rng.integers(0, 50000, size=8).tolist() for _ in range(256)]
    cases["mixed 1..128"] = [rng.integers(0, 50000, size=n).tolist()
                             for n in (1, 128, 7, 8, 9, 33, 64, 65, 100, 2, 16, 17, 31, 32, 127, 3)]
    ref = {name: encoder_ref.forward(w, seqs, device="cuda") for name, seqs in cases.items()}
    return w, cases, ref


# max |encoder - float64| over the pooled values.  Measured on the MI355X: 1.19e-6 (the mixed batch), 1.0e-6 (one token
# alone), 5.9e-7 (256 x 8), <= 3.6e-7 (single sequences of 8 .. 128 tokens); min cosine 1 - 4e-14.
E2E_BAR = 3e-6


def test_encoder_end_to_end_against_float64(enc_world, f64_world):
    """The 22-layer forward pass (every attention class alone, the bench's 256 x 8 batch, a batch of mixed lengths)
    against the float64 restatement on the same weights."""
    _, enc = enc_world
    _, cases, ref = f64_world
    worst = 0.0
    for name, seqs in cases.items():
        got = enc.encode(seqs).double()
        err = float((got - ref[name]).abs().max())
        cos = float(torch.nn.functional.cosine_similarity(got, ref[name], dim=1).min())
        print(f"{name}: max |encoder - float64| = {err:.3e}, min cosine 1 - {1 - cos:.2e}")
        worst = max(worst, err)
        assert err <= E2E_BAR, name
    print(f"end to end: max |encoder - float64| = {worst:.3e} (bar {E2E_BAR:.1e})")


def test_graph_cache_replays_other_splits_of_the_token_count(enc_world, f64_world):
    """The hipGraph cache is keyed by (token count, sequence count, normalize, length class), not by the lengths: a graph
    captured for [5, 60] must serve [60, 5], [30, 35] and [1, 64] (only the copied seq_off tells them apart), and class 8
    [3, 5] must serve [4, 4] and [5, 3].  Each replay equals the eager launch (same kernel class) bit for bit and the
    float64 model within the end-to-end bar."""
    from oracle import encoder_ref
    _, enc = enc_world
    w = f64_world[0]
    rng = np.random.default_rng(23)
    for normalize in (False, True):
        for splits in ([[5, 60], [60, 5], [30, 35], [1, 64]], [[3, 5], [4, 4], [5, 3]]):
            enc._graphs.clear()
            for lens in splits:
                seqs = [rng.integers(0, 50000, size=n).tolist() for n in lens]
                got = enc.encode(seqs, normalize=normalize)
                assert len(enc._graphs) == 1, "the first split's graph must be replayed, not a new one captured"
                enc.use_graphs = False
                try:
                    eager = enc.encode(seqs, normalize=normalize)
                finally:
                    enc.use_graphs = True
                assert torch.equal(got, eager), (normalize, lens)
                want = encoder_ref.forward(w, seqs, normalize=normalize, device="cuda")
                assert float((got.double() - want).abs().max()) <= E2E_BAR, (normalize, lens)
    enc._graphs.clear()
