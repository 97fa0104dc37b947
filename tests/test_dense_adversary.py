"""The dense filter passes restated on the CPU over adversarially rounded corpora (tests/dense_adversary.py).

Every corpus here makes |s^ - s| reach ~ eps for the planted rows, in the direction that hurts, and puts the exact top-k
within 2e-5 ... 1.5e-4 of documents the filter ranks above it.  The restated filters (f16 products or bf16 unit rows,
f32 accumulation, measured dE, tile maxima over document-cut tiles, the pass-1 sample stride, thr2, the split bound) must
keep every exact top-k document's first arg-max row with the real margin 2 eps + 1e-4 -- and the weakened variants must
lose documents, which is what makes the GPU tests on the same corpora (test_gpu_dense_filters.py) worth having."""
import numpy as np
import pytest

import dense_adversary as A

KS = (1, 10, 100)


@pytest.fixture(scope="module", params=["f16", "bf16"])
def corpus(request):
    c = A.build(request.param)
    return c, A.Filters(c)


def _exact(c, p):
    best, arg, cos = A.doc_max64(c.emb, c.doc_off, p.q)
    return best, arg, cos


def test_queries_are_their_own_normalisation_and_exact_in_both_formats():
    """prep_queries_kernel computes sum v^2 in f32 lane by lane, then a shuffle tree, and divides by sqrtf of it: with
    components x 2^-10 (|x| <= 43) every square is an integer multiple of 2^-20 below 2^-9 and every partial sum one below
    1 -- exact in f32 in ANY order -- and the sum is exactly 1, so q^ = q bit for bit.  Both 16-bit images are exact: dq = 0."""
    rng = np.random.default_rng(11)
    for _ in range(5):
        q = A.unit_query(rng)
        sq = q * q                                                   # f32
        assert np.array_equal(sq.astype(np.float64), q.astype(np.float64) ** 2)
        for order in (np.arange(A.DIM), rng.permutation(A.DIM)):
            acc = np.float32(0)
            for v in sq[order]:
                acc = np.float32(acc + v)
            assert acc == np.float32(1.0)
        lanes = sq.reshape(12, 64).sum(0, dtype=np.float32)         # lane sums, then the xor tree
        for o in (32, 16, 8, 4, 2, 1):
            lanes = (lanes + lanes[np.arange(64) ^ o]).astype(np.float32)
        assert np.all(lanes == 1.0) and np.array_equal(q / np.sqrt(lanes[0]), q)
        assert np.array_equal(A.f16(q), q) and np.array_equal(A.bf16(q), q)
        assert np.all((np.abs(q) >= 33 * 2.0 ** -10) & (np.abs(q) <= 43 * 2.0 ** -10))


def test_planted_rows_round_as_designed(corpus):
    """Corpus checks: the measured dE is attained by planted rows (filler rounds better); every designed component of a
    planted row rounds by 0.45 ulp in the designed direction (bf16: of the unit row the device builds, robustly -- no
    component within 0.04 ulp of a midpoint, norms 1 within 1e-6); the achieved |s^ - s| of every under / over row is
    >= 0.8 eps with the designed sign; twins of one group have bit-identical images."""
    c, F = corpus
    planted = c.row_role > 0
    assert F.dE_of(np.nonzero(planted)[0]) == F.dE
    assert F.dE_of(np.nonzero(~planted)[0]) < 0.9 * F.dE
    m = A.MANT[c.fmt]
    ulp = 2.0 ** (-5 - m)
    nd = A.DIM - (A.N_SLACK if c.fmt == "bf16" else 0)
    for qi, p in enumerate(c.queries):
        rows = np.nonzero(c.row_query == qi)[0]
        e = c.emb[rows].astype(np.float64)
        u = e * F.inv[rows, None] if c.fmt == "bf16" else e
        if c.fmt == "bf16":
            assert np.abs(np.linalg.norm(e, axis=1) - 1).max() < 1e-6
        d = (F.img[rows].astype(np.float64) - u)[:, :nd] * np.sign(p.q[:nd])[None, :] / ulp   # rounding, in ulps, along q
        role = c.row_role[rows]
        frac = np.abs(u[:, :nd]) / ulp % 1.0
        assert np.all(np.abs(frac - 0.5) > 0.04)
        if p.kind == "planted":
            assert np.all(np.abs(d[role == 1] + A.OFF) < 2e-3) and np.all(np.abs(d[role == 2] - A.OFF) < 2e-3)
            err = F.shat(p.q)[rows].astype(np.float64) - A.exact_cos(c.emb[rows], p.q)
            assert np.all(err[role == 1] <= -0.8 * F.dE) and np.all(err[role == 2] >= 0.8 * F.dE)
        else:
            img = F.img[rows][:, :nd]
            assert np.all(img == img[0])                                 # one image per group: a massive tie for the filter


def _sample(fmt):
    return dict(ss_div=3, ss_cap=64) if fmt == "f16" else dict(ss_div=8, ss_cap=16)


@pytest.mark.parametrize("k", KS)
def test_the_real_margin_keeps_every_exact_top_k_document(corpus, k):
    """With margin 2 eps + 1e-4 every exact top-k document's first arg-max row survives the streaming filter (both sample
    strides: the f16 pass' T / 3k <= 64 and the bf16 pass' T / 8k <= 16) and, on the bf16 corpus, the <= 128-query
    document filter.  Records how close it came: min over planted top-k documents of (s^ - cut) / margin."""
    c, F = corpus
    idx = c.of_k(k, kinds=("planted", "twins", "big"))
    assert idx
    for qi in idx:
        p = c.queries[qi]
        best, arg, _ = _exact(c, p)
        sh = F.shat(p.q)
        kept, thr, thr2, _ = A.stream_filter(sh, c.tiles, k, F.margin, **_sample(c.fmt))
        assert A.lost_docs(kept, best, arg, k) == []
        if p.kind == "planted":
            top = A.topk64(best, k)
            closest = min((sh[arg[d]] - max(thr, thr2)) / F.margin for d in top)
            assert 0.0 < closest < 0.2                                    # the corpus brings the filter near its margin
        if c.fmt == "bf16":
            assert A.lost_docs(A.doc_filter(sh, c.doc_off, k, F.margin), best, arg, k) == []


@pytest.mark.parametrize("k", KS)
def test_negative_controls_lose_documents(corpus, k):
    """Each weakened filter loses at least one exact top-k document of EVERY planted query (measured with seed 0, per
    query of k = 1 / 10 / 100: margin eps + 1e-4 loses 1 / 5 / 11 on the f16 corpus and 1 / 10 / 100 on the bf16 one --
    the bf16 document filter of <= 128 queries the same; the pass-1 threshold without its margin loses 1 / 5 / 34 and
    1 / 10 / 100); the same corpora, unweakened, lose nothing."""
    c, F = corpus
    for qi in c.of_k(k):
        p = c.queries[qi]
        best, arg, _ = _exact(c, p)
        sh = F.shat(p.q)
        half = F.margin - F.dE * 1.0001                                 # eps + 1e-4 instead of 2 eps + 1e-4
        assert A.lost_docs(A.stream_filter(sh, c.tiles, k, half, **_sample(c.fmt))[0], best, arg, k)
        nos = A.stream_filter(sh, c.tiles, k, F.margin, sample_margin_scale=0.0, **_sample(c.fmt))[0]
        assert A.lost_docs(nos, best, arg, k)
        if c.fmt == "bf16":
            assert A.lost_docs(A.doc_filter(sh, c.doc_off, k, half), best, arg, k)


def _split(c, F, p, k, part_scale):
    """msr_dense_topk_begin / _end over two shards (A: the over-documents, B: the under-documents): each vouches for
    (k_part-th largest tile maximum) - part_scale * margin, the bound is the minimum, each raises thr2 to bound - margin / 2.
    -> kept rows of the whole corpus."""
    split = int(c.doc_off[c.split_doc])
    k_part = (k + 1) // 2
    halves = []
    for lo, hi in ((0, split), (split, len(c.emb))):
        inv = F.inv[lo:hi]
        dE = A.f16_row_error(c.emb[lo:hi], inv)
        tiles = c.tiles[(c.tiles >= lo) & (c.tiles <= hi)] - lo
        sh = F.shat(p.q)[lo:hi]
        m = A.device_margin(dE)
        tmax = np.maximum.reduceat(sh, tiles[:-1])
        halves.append((lo, sh, tiles, m, A.kth_largest(tmax, k_part) - part_scale * m))
    bound = min(h[4] for h in halves)
    kept = np.zeros(len(c.emb), bool)
    for lo, sh, tiles, m, _ in halves:
        kept[lo:lo + len(sh)] = A.stream_filter(sh, tiles, k, m, bound=bound)[0]
    return kept


@pytest.mark.parametrize("k", (10, 100))
def test_split_bound_needs_the_half_margin(k):
    """The split call on the f16 corpus, k_part = ceil(k / 2): shard A's over-documents vouch for the lower part, so the
    bound comes from them.  With the real margin_scale = 1/2 nothing is lost; with 1/4 the bound exceeds the exact k-th
    score, shard B (the under-documents) raises its threshold above its lower under-documents and loses at least one
    top-k document of every planted query (measured: 4 of k = 10, 3 of k = 100).  (k = 1 cannot be attacked this way:
    shard B's one document IS sigma.)"""
    c = A.build("f16")
    F = A.Filters(c)
    for qi in c.of_k(k):
        p = c.queries[qi]
        best, arg, _ = _exact(c, p)
        assert A.lost_docs(_split(c, F, p, k, 0.5), best, arg, k) == []
        assert A.lost_docs(_split(c, F, p, k, 0.25), best, arg, k)


def test_the_slack_covers_the_f32_accumulation():
    """Why 1e-4 (5e-5 on each side of the split bound) is enough.  The filter score of a row is an f32 sum of 768 products
    (MFMA chains: v_mfma_f32_16x16x32_f16 / _bf16, 24 K steps of 32) scaled by an f32 inverse norm; the rescore
    (msr_batch_rescore_rows) is an f32 sum of 12 products per lane and a 6-level shuffle tree, times inv_norm.  With depth
    n the error of a sum is <= n u sum|a_i b_i| (u = 2^-24), and sum|a_i b_i| <= |e^| |q^| inv <= 1 + eps: counting every
    product as its own rounding (n = 768, more than any MFMA order needs) plus 4 roundings for the scaling and the norm,
    one side is off by <= 772 u (1 + 2^-7) = 4.63e-5 < 5e-5; the rescore side by <= 24 u = 1.4e-6.  The argument needs the
    slack once per side of the comparison s^(candidate) vs t^: 2 x 5e-5 = 1e-4.  On the planted rows the f32 filter sums
    (sequential order, the worst order for one-signed products) stay within that bound of the float64 products."""
    side = 772 * A.U32 * (1 + 2.0 ** -7)
    assert side < A.SLACK / 2 and 24 * A.U32 < side
    c = A.build("f16", ks=(10,), n_over_tiles=64, big=0)
    F = A.Filters(c)
    p = c.queries[0]
    rows = np.nonzero(c.row_query == 0)[0][:200]
    img, q16 = F.img[rows], A.f16(p.q)
    seq = np.zeros(len(rows), np.float32)
    for i in range(A.DIM):                                             # one f32 rounding per product and per addition
        seq = (seq + (img[:, i] * q16[i]).astype(np.float32)).astype(np.float32)
    seq = (seq * F.inv[rows]).astype(np.float32)
    exact = (img.astype(np.float64) @ q16.astype(np.float64)) * F.inv[rows].astype(np.float64)
    assert np.abs(seq - exact).max() <= side
