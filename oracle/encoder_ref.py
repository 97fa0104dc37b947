"""Float64 restatement of the query encoder (include/msretr_encoder.h).  TEST INFRASTRUCTURE ONLY.

The product runs transformers' `ModernBertModel` + sentence-transformers mean pooling as hand-written HIP
(`csrc/msr_encoder.hip`, `csrc/msr_enc_linear.hip`).  This module says the same thing in torch float64, on the layouts the
C ABI takes, so that each kernel can be compared with it and the whole forward pass with `forward`.  Line numbers cite
transformers 5.15.0: `models/modernbert/modeling_modernbert.py` (M) and `masking_utils.py` (MU).

Two steps are not float64 in transformers itself, and stay as transformers has them where they decide the result:
the rotary angle is the float32 product `t * inv_freq` (M:150-158, `.float()` on both operands), and `inv_freq` is the
float32 `1 / theta ** (arange(0, 64, 2) / 64)` (M:141).  cos / sin of that angle are taken in float64 here (M:160-161
takes them in float32; the softmax of M:180 is float32 too) -- those two are the whole difference between this module
and transformers run in float64 (tests/test_oracle_golden.py measures it).

Every function accepts numpy arrays or torch tensors and returns a float64 torch tensor on the device of its first
argument, so a test may run it on the CPU or, for the 22-layer model, on the GPU.
"""
import torch

HEAD_DIM = 64
HIDDEN, HEADS, INTER = 768, 12, 1152
GLOBAL_EVERY, THETA_GLOBAL, THETA_LOCAL, WINDOW, EPS = 3, 160000.0, 10000.0, 64, 1e-5


def _t(x, device=None, dtype=torch.float64):
    x = x if isinstance(x, torch.Tensor) else torch.as_tensor(x)
    return x.to(device=device if device is not None else x.device, dtype=dtype)


def inv_freq(theta):
    """float32 inverse frequencies of rotary embedding (M:141: `1.0 / (base ** (arange(0, dim, 2, float) / dim))`)."""
    return 1.0 / (theta ** (torch.arange(0, HEAD_DIM, 2, dtype=torch.float32) / HEAD_DIM))


def layernorm(x, w, eps=EPS):
    """torch.nn.LayerNorm(bias=False) (M:61, 312, 314, 420): (x - mean) / sqrt(biased var + eps) * w, over the last axis."""
    x = _t(x)
    w = _t(w, x.device)
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w


def layernorm_lookup(ids, table, w, eps=EPS):
    """The embedding lookup fused into the first LayerNorm (M:70: `norm(tok_embeddings(input_ids))`)."""
    table = _t(table)
    return layernorm(table[_t(ids, table.device, torch.int64)], w, eps)


def rope(x, pos, freqs):
    """Rotate-half rotary embedding (M:188-192, 217-218) of x [n, heads, 64] at integer positions pos [n].  The angle is
    the float32 product pos * inv_freq (M:150-158); cos and sin are float64."""
    x = _t(x)
    ang = (_t(pos, x.device, torch.float32)[:, None] * _t(freqs, x.device, torch.float32)[None, :]).double()
    ang = torch.cat((ang, ang), -1)[:, None, :]                                 # M:159: emb = cat(freqs, freqs)
    rot = torch.cat((-x[..., HEAD_DIM // 2:], x[..., :HEAD_DIM // 2]), -1)      # rotate_half
    return x * torch.cos(ang) + rot * torch.sin(ang)


def positions(seq_off, run_on=False):
    """Token positions of a packed batch: 0 .. S-1 in every sequence (M:449 gives every padded row arange(seq_len)).
    run_on=True numbers the tokens of the whole pack 0 .. n_tok-1 instead -- a deliberate error for negative controls."""
    off = [int(v) for v in _t(seq_off, None, torch.int64).cpu()]
    if run_on:
        return torch.arange(off[-1])
    return torch.cat([torch.arange(e - s) for s, e in zip(off[:-1], off[1:])] + [torch.zeros(0, dtype=torch.int64)])


def attention(qkv, seq_off, n_heads, freqs, window, run_on_positions=False):
    """msr_enc_attention.  qkv [n_tok][3][n_heads][64] (any shape with that element order), sequence b = tokens
    [seq_off[b], seq_off[b+1]).  Rotary embedding of q and k at the token's position in its sequence; scores q.k * 64**-0.5
    (M:176, 293); key k is kept for query t iff window <= 0 or |t - k| <= window (MU:141-151,
    `sliding_window_bidirectional_overlay` with config.sliding_window = 64; the `+ 1` of M:253 goes to the flash-attention
    kwargs only, the eager / sdpa mask is built from the config); softmax over the kept keys (M:180), times v.
    Returns [n_tok][n_heads * 64]."""
    qkv = _t(qkv)
    n_tok = qkv.numel() // (3 * n_heads * HEAD_DIM)
    qkv = qkv.reshape(n_tok, 3, n_heads, HEAD_DIM)
    pos = positions(seq_off, run_on_positions).to(qkv.device)
    q = rope(qkv[:, 0], pos, freqs)
    k = rope(qkv[:, 1], pos, freqs)
    v = qkv[:, 2]
    out = torch.zeros(n_tok, n_heads, HEAD_DIM, dtype=torch.float64, device=qkv.device)
    off = [int(x) for x in _t(seq_off, None, torch.int64).cpu()]
    by_len = {}                                                  # sequences of one length go through as one batch
    for s, e in zip(off[:-1], off[1:]):
        if e > s:
            by_len.setdefault(e - s, []).append(s)
    for S, starts in by_len.items():
        idx = (torch.tensor(starts)[:, None] + torch.arange(S)[None, :]).to(qkv.device)          # [B, S]
        qb, kb, vb = (z[idx].transpose(1, 2) for z in (q, k, v))                                # [B, H, S, 64]
        sc = qb @ kb.transpose(-1, -2) * HEAD_DIM ** -0.5
        if window > 0:
            d = (torch.arange(S)[:, None] - torch.arange(S)[None, :]).abs().to(qkv.device)
            sc = sc.masked_fill(d > window, float("-inf"))
        out[idx] = (torch.softmax(sc, -1) @ vb).transpose(1, 2)
    return out.reshape(n_tok, n_heads * HEAD_DIM)


def geglu(u):
    """msr_enc_geglu / ModernBertMLP (M:90-91): gelu(u[:, :half]) * u[:, half:], exact-erf GELU (hidden_activation "gelu")."""
    u = _t(u)
    half = u.shape[-1] // 2
    a, g = u[..., :half], u[..., half:]
    return 0.5 * a * (1.0 + torch.erf(a / 2 ** 0.5)) * g


def mean_pool(h, seq_off, normalize=False):
    """msr_enc_mean_pool: mean of each sequence's rows (sentence-transformers Pooling, mean mode); an empty sequence gives
    a zero vector.  normalize: divided by max(||mean||, 1e-12) (torch.nn.functional.normalize)."""
    h = _t(h)
    off = [int(x) for x in _t(seq_off, None, torch.int64).cpu()]
    out = torch.zeros(len(off) - 1, h.shape[-1], dtype=torch.float64, device=h.device)
    for b, (s, e) in enumerate(zip(off[:-1], off[1:])):
        if e > s:
            out[b] = h[s:e].mean(0)
    if normalize:
        out = out / out.norm(dim=1, keepdim=True).clamp(min=1e-12)
    return out


def forward(weights, seqs, layers=None, normalize=False, device="cpu", window=WINDOW, run_on_positions=False):
    """The whole encoder on packed sequences (lists of token ids) -> pooled float64 [len(seqs), 768].

    weights: the Hugging Face parameter names QueryEncoder takes (a leading "model." is ignored).  Layer schedule as in
    encoder.py / ModernBertConfig: layer l is global (no window, theta 160000) iff l % 3 == 0, otherwise local (window 64,
    theta 10000); layer 0 has no attn_norm (M:309-310).  Per layer (M:325-333):
        h += Wo . attention(Wqkv . attn_norm(h));  h += mlp.Wo . geglu(Wi . mlp_norm(h))
    then final_norm (M:476) and mean pooling.  `window` and `run_on_positions` exist for the negative controls of the tests
    (the local window's half width, and positions that do not restart per sequence)."""
    w = {(k[len("model."):] if k.startswith("model.") else k): _t(v, device) for k, v in weights.items()}
    if layers is None:
        layers = 1 + max(int(k.split(".")[1]) for k in w if k.startswith("layers."))
    off = [0]
    for s in seqs:
        off.append(off[-1] + len(s))
    ids = torch.tensor([t for s in seqs for t in s], dtype=torch.int64)
    freqs = {True: inv_freq(THETA_GLOBAL), False: inv_freq(THETA_LOCAL)}
    h = layernorm_lookup(ids, w["embeddings.tok_embeddings.weight"], w["embeddings.norm.weight"])
    for l in range(layers):
        p = f"layers.{l}."
        glob = l % GLOBAL_EVERY == 0
        x = h if l == 0 else layernorm(h, w[p + "attn_norm.weight"])
        qkv = x @ w[p + "attn.Wqkv.weight"].T
        att = attention(qkv, off, HEADS, freqs[glob], 0 if glob else window, run_on_positions)
        h = h + att @ w[p + "attn.Wo.weight"].T
        h = h + geglu(layernorm(h, w[p + "mlp_norm.weight"]) @ w[p + "mlp.Wi.weight"].T) @ w[p + "mlp.Wo.weight"].T
    h = layernorm(h, w["final_norm.weight"])
    return mean_pool(h, off, normalize)
