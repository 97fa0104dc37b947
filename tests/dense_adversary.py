"""Dense corpora that drive the filter passes of the dense stage to their margins (DESIGN section 3 K2+K3 / K5, section 4).

TEST INFRASTRUCTURE ONLY, CPU, deterministic from a seed (numpy; torch for bf16 round-to-nearest-even as __bf16 does).

The streaming passes and the batched path score every (row, query) pair approximately -- f16(e) . f16(q^) or
bf16(e / |e|) . bf16(q^), f32 accumulation -- and keep what lies above (a lower bound of the k-th approximate score t^)
- margin, margin = 2 eps + 1e-4, eps = dE (1 + dq) + dq from MEASURED rounding errors.  On random rows the rounding errors
point in random directions and |s^ - s| is a small fraction of eps.  Here they do not:

* queries have components x_i 2^-10 with integers 33 <= |x_i| <= 43 and sum x_i^2 = 2^20: the device normalises them to
  themselves (every square and partial sum is exact in f32, sqrtf(1) = 1) and their f16 and bf16 images are exact, so
  dq = 0 and eps = dE;
* a planted row of query q has every magnitude on the grid of the target format inside one binade, [2^-5, 2^-4), plus
  t ulp along sign(q_i): e_i = sign(q_i) (j_i ulp + t ulp).  t = +0.45 ("under"): the rounded row loses 0.45 ulp
  against q in every component, s^ ~ s - eps; t = -0.45 ("over"): s^ ~ s + eps.  For bf16 the device rounds e / |e|:
  the row norm is fixed to 1 with two slack components so that 1 / |e| moves no component across a rounding midpoint;
* per planted query and its k: k under-documents at and above sigma (exact scores at least GAP apart; f16: the best
  half of them 3 eps higher) in one half of the corpus, an over-document 2e-5 ... 1.5e-4 below sigma in EVERY tile of the other half -- they lift t^ to ~ sigma + eps
  while the under-documents sink to ~ sigma - eps.  Each planted document is alone (for its query) in a row tile of
  256 rows, so tile maxima are document maxima;
* twins: documents whose rows round to the SAME f16 / bf16 vector with different exact cosines (t on a ladder in
  [-0.4, 0.4]), bit-identical rows in different documents and inside one document; one small group (fits the
  candidate buffers) and one of 5500 documents (more than GF_PAIR_CAP = MSR_SEL_CAP = 4096);
* filler: random rows of norm 0.6 ... 1.8 (relative rounding error below the planted rows'), documents of 1 ... 60 rows,
  chunk-less documents (leading, inside, trailing).
"""
from dataclasses import dataclass, field

import numpy as np
import torch

DIM = 768
U32 = 2.0 ** -24                          # f32 unit roundoff
MANT = {"f16": 10, "bf16": 7}             # explicit significand bits of the target format
OFF = 0.45                                # planted rounding offset, in ulps of the target format
SLACK = 1e-4                              # the margin's slack (f16_margin_kernel, batch_margin_kernel)
GAP = 2e-5                                # least distance between exact scores of documents next to each other in a top-k
OVER_LO, OVER_HI = 1.5e-4, 2e-5           # over-documents lie this far below sigma
TILE = 256                                # rows per tile of the streaming passes (msr_bind_chunks cuts tiles greedily)
N_SLACK = 2                               # bf16 rows: components that fix the norm to 1


# ------------------------------------------------------------------------------------------------ rounding
def f16(x):
    return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


def bf16(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def inv_norm(emb):
    n = np.sqrt(np.einsum("ij,ij->i", emb, emb, dtype=np.float64))
    return (1.0 / np.where(n == 0, 1.0, n)).astype(np.float32)


def f16_row_error(emb, inv):
    """f16_row_error_kernel: max_r |e_r - f16(e_r)| / |e_r|, a value that converts to an f16 subnormal counted as lost."""
    h = f16(emb)
    d = np.where(np.abs(h) < 2.0 ** -14, emb, h - emb).astype(np.float64)
    return float(np.max(np.sqrt(np.einsum("ij,ij->i", d, d)) * inv))


def unit_bf16(emb, inv):
    """unit_bf16_rows_kernel: bf16(e * inv_norm) and dE = max_r |bf16(u_r) - u_r|."""
    u = (emb * inv[:, None]).astype(np.float32)
    b = bf16(u)
    d = (b - u).astype(np.float64)
    return b, float(np.max(np.sqrt(np.einsum("ij,ij->i", d, d))))


def device_margin(dE, dq=0.0):
    """f16_margin_kernel / batch_margin_kernel, in f64."""
    dq, dE = dq * 1.0001, dE * 1.0001
    return 2.0 * (dE * (1.0 + dq) + dq * 1.000001) + SLACK


# ------------------------------------------------------------------------------------------------ queries
def unit_query(rng):
    """Components x_i 2^-10, integers 33 <= |x_i| <= 43, sum x_i^2 = 2^20 exactly, random signs."""
    target = 1 << 20
    x = np.clip(np.rint(rng.normal(37.0, 3.0, DIM)), 33, 43).astype(np.int64)
    while abs(int(x @ x) - target) > 400:
        d = int(x @ x) - target
        i = rng.integers(0, DIM, 64)
        step = -1 if d > 0 else 1
        ok = (x[i] + step >= 33) & (x[i] + step <= 43)
        i = np.unique(i[ok])[:max(1, min(64, abs(d) // 80))]
        x[i] += step
    vals = np.arange(33, 44)
    sq = vals ** 2
    four = sq[:, None, None, None] + sq[None, :, None, None] + sq[None, None, :, None] + sq[None, None, None, :]
    while True:
        pos = rng.choice(DIM, 4, replace=False)
        need = target - (int(x @ x) - int(x[pos] @ x[pos]))
        hit = np.argwhere(four == need)
        if len(hit):
            x[pos] = vals[hit[rng.integers(len(hit))]]
            break
    assert int(x @ x) == target
    sign = np.where(rng.random(DIM) < 0.5, -1, 1)
    return (sign * x * 2.0 ** -10).astype(np.float32)


# ------------------------------------------------------------------------------------------------ planted rows
def _grid(fmt):
    m = MANT[fmt]
    return 1 << m, 1 << (m + 1), 1 << (23 - m)     # grid ints of the binade [lo, hi), f32 units (2^-28) per ulp


def base_grid(rng, q, n, fmt):
    """n grid vectors j (ints, magnitudes j ulp in [2^-5, 2^-4)) near |q|: a blend of |q| with a permutation of itself."""
    lo, hi, _ = _grid(fmt)
    jq = np.rint(np.abs(q.astype(np.float64)) * 2.0 ** (5 + MANT[fmt])).astype(np.int64)   # |q_i| on the grid
    beta = rng.uniform(0.0, 1.0, (n, 1))
    perm = jq[np.argsort(rng.random((n, DIM)), axis=1)]
    j = np.rint((1.0 - beta) * jq[None, :] + beta * perm).astype(np.int64)
    return np.clip(j, lo + 1, hi - 2)


def _values(sgn, j, t, fmt):
    """e_i = sgn_i (j_i + t_i) ulp in f32 (t in ulps per row or per component, rounded to f32 units: exact)."""
    _, _, uu = _grid(fmt)
    t = np.asarray(t, np.float64)
    n = j * uu + np.rint((t if t.ndim == 2 else t.reshape(-1, 1)) * uu).astype(np.int64)
    assert n.max() < (1 << 24) and n.min() >= (1 << 23)
    return (sgn.astype(np.float64) * n * 2.0 ** -28).astype(np.float32)


def fix_unit_norm(rng, sgn, j, t):
    """bf16 rows: adjust the grid ints so that sum_designed e^2 ~ 1 - 2 v^2 (v ~ 0.0475), then set the last N_SLACK
    components to sign(q_i) v with v = sqrt((1 - sum_designed e^2) / 2): |e| = 1 within ~1e-9.  -> (j, slack values)."""
    lo, hi, _ = _grid("bf16")
    want = 1.0 - N_SLACK * 0.0475 ** 2
    d = slice(0, DIM - N_SLACK)
    for _ in range(8):
        e = _values(sgn, j, t, "bf16").astype(np.float64)
        S = np.einsum("ij,ij->i", e[:, d], e[:, d])
        grad = 2.0 * np.abs(e[:, d]).sum(1) * 2.0 ** -12
        step = (want - S) / grad
        j[:, d] += np.floor(step[:, None] + rng.random((len(j), DIM - N_SLACK))).astype(np.int64)
        j = np.clip(j, lo + 1, hi - 2)
    e = _values(sgn, j, t, "bf16").astype(np.float64)
    S = np.einsum("ij,ij->i", e[:, d], e[:, d])
    v = np.sqrt((1.0 - S) / N_SLACK)
    assert np.all((v >= 2.0 ** -5) & (v < 2.0 ** -4)), "slack outside the binade"
    return j, v.astype(np.float32)


def rows_of(sgn, j, t, fmt, slack=None):
    e = _values(sgn, j, t, fmt)
    if fmt == "bf16":
        e[:, DIM - N_SLACK:] = (sgn[DIM - N_SLACK:][None, :] * slack[:, None]).astype(np.float32)
    return e


def planted_pool(rng, q, n, t, fmt):
    j = base_grid(rng, q, n, fmt)
    slack = None
    if fmt == "bf16":
        j, slack = fix_unit_norm(rng, np.sign(q), j, np.full(n, t))
    return rows_of(np.sign(q), j, np.full(n, t), fmt, slack)


def exact_cos(rows, q):
    r = rows.astype(np.float64)
    return (r @ q.astype(np.float64)) / np.sqrt(np.einsum("ij,ij->i", r, r)) / np.linalg.norm(q.astype(np.float64))


# ------------------------------------------------------------------------------------------------ the corpus
@dataclass
class Planted:
    q: np.ndarray                 # float32 [768]
    k: int
    kind: str                     # "planted" | "twins" | "big"
    sigma: float = 0.0            # exact k-th score (planted)
    docs: list = field(default_factory=list)     # [(rows float32 [r, 768], role)] role: "under" | "over" | "twin"


@dataclass
class Corpus:
    fmt: str
    emb: np.ndarray               # float32 [C, 768]
    doc_off: np.ndarray           # int64 [N + 1]
    tiles: np.ndarray             # int64 row boundaries of the streaming passes' tiles
    queries: list                 # [Planted]
    row_query: np.ndarray         # int32 [C]: planted query a row belongs to, -1 filler
    row_role: np.ndarray          # int8 [C]: 0 filler, 1 under, 2 over, 3 twin
    split_doc: int                # first document of the second half (shard B: under-documents, twins)

    @property
    def n_docs(self):
        return len(self.doc_off) - 1

    def qmat(self, idx):
        return np.stack([self.queries[i].q for i in idx])

    def of_k(self, k, kinds=("planted",)):
        return [i for i, p in enumerate(self.queries) if p.k == k and p.kind in kinds]


def greedy_tiles(doc_off):
    """msr_bind_chunks: tiles of <= 256 rows cut at document boundaries, greedily."""
    doc_off = np.asarray(doc_off, np.int64)
    tiles, start = [0], 0
    for d in range(len(doc_off) - 1):
        if doc_off[d + 1] - start > TILE:
            tiles.append(int(doc_off[d])); start = int(doc_off[d])
    if tiles[-1] != doc_off[-1]:
        tiles.append(int(doc_off[-1]))
    return np.asarray(tiles, np.int64)


def _ladder(order, su, start, n):
    pick = [order[start]]
    for i in order[start + 1:]:
        if len(pick) == n:
            break
        if su[i] >= su[pick[-1]] + GAP:
            pick.append(i)
    assert len(pick) == n, "under pool too narrow"
    return pick


def _planted_query(rng, k, fmt):
    """k under-documents at and above sigma, GAP apart; over-documents OVER_HI ... OVER_LO below sigma (highest first).
    f16: the best ceil(k / 2) under-documents lie 3 eps above the others, so that a shard holding the under-documents
    vouches for a HIGHER bound than one holding the over-documents (the split call's bound then comes from the latter)."""
    q = unit_query(rng)
    n_pool = 4000 if k < 100 else 6000
    under = planted_pool(rng, q, n_pool, +OFF, fmt)
    su = exact_cos(under, q)
    order = np.argsort(su)
    start = int(0.05 * n_pool)
    if fmt == "f16" and k >= 2:
        e = under.astype(np.float64)
        eps = float(np.max(np.linalg.norm(f16(under) - e, axis=1) / np.linalg.norm(e, axis=1)))
        n_hi = (k + 1) // 2
        pick = _ladder(order, su, start, k - n_hi)
        hi0 = int(np.searchsorted(su[order], su[pick[-1]] + 3.0 * eps))
        pick += _ladder(order, su, hi0, n_hi)
    else:
        pick = _ladder(order, su, start, k)
    sigma = float(su[pick[0]])
    over = planted_pool(rng, q, n_pool, -OFF, fmt)
    so = exact_cos(over, q)
    ok = np.nonzero((so <= sigma - OVER_HI) & (so >= sigma - OVER_LO))[0]
    assert len(ok) >= 8, "over pool too narrow"
    ok = ok[np.argsort(-so[ok])]
    p = Planted(q=q, k=k, kind="planted", sigma=sigma)
    p.docs = [(under[i:i + 1], "under") for i in pick]
    p.over = [over[i:i + 1] for i in ok]
    return p


def _twin_rows(rng, q, ts, fmt):
    """Rows that round to ONE vector of the format, with exact cosines spread by t: a common grid vector with 10 % of its
    signs flipped against q (cosine ~0.8: a row parallel to q would barely turn with t), offsets t ulp along the signs of
    the part of q orthogonal to it -- the direction in which the offset moves the cosine most (~2e-4 per ulp for f16)."""
    j = base_grid(rng, q, 1, fmt)
    sgn = np.sign(q) * np.where(rng.random(DIM) < 0.1, -1, 1)
    if fmt == "bf16":
        sgn[DIM - N_SLACK:] = np.sign(q[DIM - N_SLACK:])
    e = _values(sgn, j, np.zeros(1), fmt)[0].astype(np.float64)
    eh = e / np.linalg.norm(e)
    w = np.sign(q - (eh @ q) * eh) * sgn                              # offset direction, in units along sgn
    ts = np.asarray(ts, np.float64)
    t = ts[:, None] * w[None, :]
    slack = None
    if fmt == "bf16":
        t[:, DIM - N_SLACK:] = 0.0
        j, _ = fix_unit_norm(rng, sgn, j.copy(), np.zeros((1, DIM)))
        e = _values(sgn, np.repeat(j, len(ts), 0), t, fmt).astype(np.float64)[:, :DIM - N_SLACK]
        slack = np.sqrt((1.0 - np.einsum("ij,ij->i", e, e)) / N_SLACK).astype(np.float32)   # every twin of norm 1
    return rows_of(sgn, np.repeat(j, len(ts), 0), t, fmt, slack)


def build(fmt="f16", seed=0, ks=(1, 1, 10, 10, 100), n_over_tiles=128, big=5500):
    """The adversarial corpus of one format.  Layout: [leading chunk-less document] [half A: n_over_tiles tiles, each with
    one over-document of every planted query] [half B: the under-documents, one per tile and query; the small twin group,
    one document per tile; the big twin group, 256 documents per tile] [trailing chunk-less document]; filler documents
    fill every tile to exactly 256 rows, so the greedy cut reproduces the tiles."""
    rng = np.random.default_rng(seed)
    queries = [_planted_query(rng, k, fmt) for k in ks]
    # small twin group (k = 10): 8 ladder levels; two more documents bit-identical to the top level; one document of two
    # identical rows equal to the second level (exact ties between documents and inside one)
    tq = unit_query(rng)
    top_t = 0.4 if fmt == "f16" else 0.2         # (bf16: the slack that keeps every twin at norm 1 bends the ladder above ~0.3)
    ladder = np.linspace(-0.4, top_t, 8)
    tr = _twin_rows(rng, tq, ladder, fmt)
    ts = exact_cos(tr, tq)
    top, second = np.argsort(-ts)[:2]
    tw = Planted(q=tq, k=10, kind="twins")
    tw.docs = [(tr[i:i + 1], "twin") for i in range(len(ladder))]
    assert np.all(np.abs(np.diff(np.sort(ts))) >= GAP), "twin ladder too narrow"
    tw.docs += [(tr[top:top + 1].copy(), "twin"), (tr[top:top + 1].copy(), "twin"), (np.repeat(tr[second:second + 1], 2, 0), "twin")]
    rng.shuffle(tw.docs)
    queries.append(tw)
    # big twin group (k = 10): 5 levels x 1100 bit-identical documents, interleaved
    bq = unit_query(rng)
    lv = _twin_rows(rng, bq, np.linspace(-0.4, top_t, 5), fmt)
    assert np.all(np.abs(np.diff(np.sort(exact_cos(lv, bq)))) >= GAP)
    bg = Planted(q=bq, k=10, kind="big")
    level = rng.permutation(np.arange(big) % 5)
    big_rows = lv[level]
    queries.append(bg)

    docs, roles, owners = [], [], []          # per document: rows, role id, owner query (-1 filler)

    def filler(n_rows):
        if n_rows == 0:
            return []
        out = []
        left = n_rows
        while left > 0:
            r = int(min(left, rng.integers(1, 61)))
            out.append(r)
            left -= r
        return out

    def emit_tile(planted_docs):
        """planted_docs: [(rows, role, owner)] -> one tile of exactly 256 rows, planted documents at random places."""
        used = sum(len(r) for r, _, _ in planted_docs)
        items = [("p", x) for x in planted_docs] + [("f", n) for n in filler(TILE - used)]
        order = rng.permutation(len(items))
        for i in order:
            kind, x = items[i]
            if kind == "p":
                docs.append(x[0]); roles.append(x[1]); owners.append(x[2])
            else:
                docs.append(x); roles.append(0); owners.append(-1)
            if rng.random() < 0.01:
                docs.append(0); roles.append(0); owners.append(-1)       # a chunk-less document inside the corpus

    role_id = {"under": 1, "over": 2, "twin": 3}
    docs.append(0); roles.append(0); owners.append(-1)                   # leading chunk-less document
    for t in range(n_over_tiles):
        emit_tile([(p.over[t % len(p.over)], 2, qi) for qi, p in enumerate(queries) if p.kind == "planted"])
    split_doc = len(docs)
    n_b = max(max(len(p.docs) for p in queries if p.kind != "big"), 64)
    for t in range(n_b):
        pd = [(p.docs[t][0], role_id[p.docs[t][1]], qi) for qi, p in enumerate(queries) if p.kind != "big" and t < len(p.docs)]
        emit_tile(pd)
    for s in range(0, big, TILE):
        for r in range(s, min(big, s + TILE)):
            docs.append(big_rows[r:r + 1]); roles.append(3); owners.append(len(queries) - 1)
        if big - s < TILE:
            docs.append(TILE - (big - s)); roles.append(0); owners.append(-1)
    docs.append(0); roles.append(0); owners.append(-1)                   # trailing chunk-less document

    sizes = np.array([len(d) if not isinstance(d, int) else d for d in docs], np.int64)
    doc_off = np.zeros(len(docs) + 1, np.int64)
    doc_off[1:] = np.cumsum(sizes)
    C = int(doc_off[-1])
    emb = np.empty((C, DIM), np.float32)
    row_query = np.full(C, -1, np.int32)
    row_role = np.zeros(C, np.int8)
    fill = np.ones(C, bool)
    for d, x in enumerate(docs):
        if not isinstance(x, int):
            a = doc_off[d]
            emb[a:a + len(x)] = x
            fill[a:a + len(x)] = False
            row_query[a:a + len(x)] = owners[d]
            row_role[a:a + len(x)] = roles[d]
    nf = int(fill.sum())
    g = rng.standard_normal((nf, DIM), dtype=np.float32)
    g *= (rng.uniform(0.6, 1.8, (nf, 1)) / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32)
    emb[fill] = g
    tiles = greedy_tiles(doc_off)
    c = Corpus(fmt=fmt, emb=emb, doc_off=doc_off, tiles=tiles, queries=queries, row_query=row_query, row_role=row_role,
               split_doc=split_doc)
    _check_layout(c)
    return c


def _check_layout(c):
    """Every tile is 256 rows; no tile holds two documents of one planted query; the halves split at a tile boundary."""
    sizes = np.diff(c.tiles)
    assert np.all(sizes[:-1] == TILE) and sizes[-1] <= TILE
    assert np.all(np.diff(c.doc_off) <= TILE)
    split_row = c.doc_off[c.split_doc]
    assert split_row in set(c.tiles.tolist())
    tile_of = np.searchsorted(c.tiles, np.arange(len(c.emb)), side="right") - 1
    doc_of = np.searchsorted(c.doc_off, np.arange(len(c.emb)), side="right") - 1
    for qi, p in enumerate(c.queries):
        if p.kind == "big":
            continue
        rows = np.nonzero(c.row_query == qi)[0]
        t_docs = {}
        for r in rows:
            t_docs.setdefault(int(tile_of[r]), set()).add(int(doc_of[r]))
        assert all(len(v) == 1 for v in t_docs.values()), "two planted documents of one query share a tile"


# ------------------------------------------------------------------------------------------------ float64 reference
def doc_max64(emb, doc_off, q, max_chunks=0):
    """-> (best float64 [N] (-inf: no rows), first arg-max row int64 [N] (-1), cosine per row float64 [C])."""
    doc_off = np.asarray(doc_off, np.int64)
    N, C = len(doc_off) - 1, int(doc_off[-1])
    q64 = q.astype(np.float64) / np.linalg.norm(q.astype(np.float64))
    cos = np.empty(C, np.float64)
    for s in range(0, C, 65536):
        r = emb[s:s + 65536].astype(np.float64)
        n = np.sqrt(np.einsum("ij,ij->i", r, r))
        cos[s:s + 65536] = (r @ q64) / np.where(n == 0, 1.0, n)
    n_rows = np.diff(doc_off)
    doc = np.repeat(np.arange(N), n_rows)
    if max_chunks > 0:
        pos = np.arange(C) - np.repeat(doc_off[:-1], n_rows)
        cos_m = np.where(pos < max_chunks, cos, -np.inf)
    else:
        cos_m = cos
    best = np.full(N, -np.inf)
    nz = np.nonzero(n_rows > 0)[0]
    best[nz] = np.maximum.reduceat(cos_m, doc_off[nz])
    is_max = cos_m == best[doc]
    arg = np.full(N, C, np.int64)
    np.minimum.at(arg, doc[is_max], np.nonzero(is_max)[0])
    arg[arg == C] = -1
    return best, arg, cos


def topk64(best, k):
    """(score desc, index asc) over documents with rows."""
    ok = np.nonzero(np.isfinite(best))[0]
    order = ok[np.lexsort((ok, -best[ok]))]
    return order[:k]


# ------------------------------------------------------------------------------------------------ restated filters
def kth_largest(v, k):
    v = v[np.isfinite(v)]
    return np.partition(v, len(v) - k)[len(v) - k] if len(v) >= k else np.inf


def stream_filter(shat, tiles, k, margin, ss_div=3, ss_cap=64, sample_margin_scale=1.0, bound=None, bound_margin_scale=0.5):
    """The streaming passes' kept rows (msr_gemm_f32_pass / msr_gemm_candidates + finish): pass 1 thresholds at the k-th
    largest maximum of every ss-th tile (ss = clamp(T / (ss_div k), 1, ss_cap), tiles ss/2, ss/2 + ss, ...) minus the
    margin and emits s^ >= thr; the bucket keeps s^ >= thr2 = (k-th largest of all tile maxima) - margin, raised to
    bound - margin / 2 by a cross-shard bound.  -> (kept rows bool, thr, thr2, tile maxima)."""
    tmax = np.maximum.reduceat(shat, tiles[:-1])
    T = len(tmax)
    ss = min(max(T // (ss_div * k), 1), ss_cap)
    sampled = tmax[ss // 2::ss]
    thr = kth_largest(sampled, k) - sample_margin_scale * margin
    thr2 = kth_largest(tmax, k) - margin
    if bound is not None:
        thr2 = max(thr2, bound - bound_margin_scale * margin)
    return (shat >= thr) & (shat >= thr2), thr, thr2, tmax


def doc_filter(shat, doc_off, k, margin):
    """The <= 128-query batched path (bf16 K-split sweep + msr_batch_finish): candidates = documents whose approximate
    max-cosine is >= (k-th largest of them) - margin; all their rows are rescored.  -> kept rows bool."""
    doc_off = np.asarray(doc_off, np.int64)
    n_rows = np.diff(doc_off)
    nz = np.nonzero(n_rows > 0)[0]
    dmax = np.full(len(n_rows), -np.inf, np.float32)
    dmax[nz] = np.maximum.reduceat(shat, doc_off[nz])
    cut = kth_largest(dmax, k) - margin
    return np.repeat(dmax >= cut, n_rows)


def lost_docs(kept, best, arg, k):
    """Exact top-k documents whose first arg-max row was not kept."""
    top = topk64(best, k)
    return [int(d) for d in top if not kept[arg[d]]]


class Filters:
    """The approximate scores of one corpus as the device computes them, with the measured margins."""

    def __init__(self, c):
        self.c = c
        self.inv = inv_norm(c.emb)
        if c.fmt == "f16":
            self.img = f16(c.emb)
            self.dE = f16_row_error(c.emb, self.inv)
            self.dE_rows = None
        else:
            self.img, self.dE = unit_bf16(c.emb, self.inv)
        self.margin = device_margin(self.dE)

    def shat(self, q):
        qn = q.astype(np.float32)            # the planted queries are their own normalisation, exact in both formats
        if self.c.fmt == "f16":
            return ((self.img @ f16(qn)) * self.inv).astype(np.float32)
        return (self.img @ bf16(qn)).astype(np.float32)

    def dE_of(self, rows):
        if self.c.fmt == "f16":
            return f16_row_error(self.c.emb[rows], self.inv[rows])
        return unit_bf16(self.c.emb[rows], self.inv[rows])[1]
