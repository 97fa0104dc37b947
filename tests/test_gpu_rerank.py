"""The rerank kernels (csrc/msr_rerank.hip) against the CPU restatement, bit for bit where the
arithmetic is the reference's, within a derived bar where it is the gather's f32.

Fuse (B): all float64, -ffp-contract=off, the reference's operations in its order -- so DeviceEngine.rerank_fuse on
hand-built cos / meta must return exactly what rerank_ref.fuse_from_gather returns: documents, score and orig as float64
bits, chunk rows, n and rows (cases: tests/rerank_cases.py; test_rerank_exact.py shows each restated wrong fuse fails
one of them).

Gather (A): cosine = (sum over 768 dims of e_i * qn_i) * inv_norm[row], in f32, against the float64 cosine with sklearn's
zero-norm-to-1 rule.  Bar (u = 2^-24; gamma_k <= k u (1 + k u)):
  * qn = q / |q|^ (prep_queries_kernel): |q|^2 is 12 squares summed one after the other per lane, then a 6-level butterfly:
    every square passes <= 1 + 11 + 6 = 18 roundings, relative error <= gamma_18; sqrtf and the division within 1 ulp (2u)
    each.  The norm's error is ONE factor common to every qn_i, (1 + nu) with |nu| <= 9u + 2u = 11u; each qn_i adds its own
    division, 2u.
  * s = sum e_i qn_i (rerank_cos_kernel): 12 products per lane summed in order (3 groups of 4), then the 6-level butterfly:
    each product passes 1 + 11 + 6 = 18 roundings, |s^ - s| <= gamma_18 sum |e_i qn_i|.
  * times inv_norm: one rounding (u), and inv_norm's own relative error eta.  Layout 0 computes it in row_inv_norm_kernel
    the same way as |q| (18 roundings in the sum, sqrtf, 1 / nrm): |eta| <= 9u + 2u + 2u = 13u.  Layout 1 binds torch's
    1 / vector_norm: eta is MEASURED per row from the tensor the engine bound, |inv (float64 |e|) - 1|.
  Together, with c the exact cosine and A = sum |e_i q_i| / (|e| |q|) <= 1:
      |cos^ - c| <= u (20 A + 12 |c|) + |eta| |c|,     times (1 + 64 u) for the second-order terms
  (rerank_cases.gather_bar: GATHER_A = 18 + 2, GATHER_B = 11 + 1).  A zero row has inv_norm 1 and s = 0: exactly 0.

End to end (DeviceEngine.rerank, max_queries=8: msr_rerank slices by 128 queries): equal to fuse_from_gather on the
gather's own output, bit for bit; against the chain on float64 cosines: new = (c - cmin) / (cmax - cmin) moves by
  dnew = ((1 - new)(dc - dcmin) + new (dc - dcmax)) / (cmax - cmin),   |dnew| <= 2 bar_max / (cmax - cmin)
with bar_max the largest cosine bar among the query's kept rows; the blend scales it by (1 - smoothing), the positional
shift and the clamps do not grow it, a maximum over rows neither.  The float64 chain itself rounds a handful of operations
on values of magnitude <= 1 + max_boost (subtract, divide, two products, two sums, the shift): 16 U64 covers them.  So
      |score^ - score| <= (1 - smoothing) 2 bar_max / (cmax - cmin) (1 + 64 u) + 16 U64 =: sbar
unless the document's best row changes; a changed best row (before or after the positional shift), or two documents in
the other order, must be explained by two float64 values within 2 sbar.
"""
import numpy as np
import pytest

import rerank_cases as RC
from oracle import rerank_ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

U32 = RC.U32
FRACTIONS = {}


@pytest.fixture(scope="module")
def mods():
    from msretr.engine import DeviceEngine
    from msretr.index import CorpusIndex
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return dict(DeviceEngine=DeviceEngine, CorpusIndex=CorpusIndex)


@pytest.fixture(scope="module")
def z():
    z = RC.gather_corpus()
    z["c64"], z["A"] = RC.cos64(z["queries"], z["emb"])
    return z


_ENG = {}


def _index(mods, z, d0=0, d1=None):
    d1 = z["N"] if d1 is None else d1
    off = z["doc_off"][d0:d1 + 1] - z["doc_off"][d0]
    r0, r1 = int(z["doc_off"][d0]), int(z["doc_off"][d1])
    return mods["CorpusIndex"](doc_ids=np.arange(d0, d1, dtype=np.int64), doc_off=off.astype(np.int32),
                               chunk_ids=np.arange(r0, r1, dtype=np.int64), emb=z["emb"][r0:r1], total_docs=z["N"],
                               doc_base=d0, row_base=r0, _url_group=z["url_group"][d0:d1].copy())


def _engine(mods, z, layout=0, max_queries=32, d0=0, d1=None):
    key = (layout, max_queries, d0, d1)
    if key not in _ENG:
        _ENG[key] = mods["DeviceEngine"](_index(mods, z, d0, d1), device=0, max_queries=max_queries, max_k=100,
                                         rerank_max_docs=RC.M, scan_layout=layout)
    return _ENG[key]


def teardown_module(module):
    for e in _ENG.values():
        e.close()
    _ENG.clear()
    for k, v in sorted(FRACTIONS.items()):
        print(f"rerank bar: {k}: largest error / bar = {v:.4f}")


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


# ------------------------------------------------------------------ fuse (B), bit for bit
def _fuse_gpu(eng, cases):
    prm = cases[0]["prm"]
    assert all(c["prm"] == prm for c in cases)
    st = lambda k: np.stack([c[k] for c in cases])
    out = eng.rerank_fuse(st("doc"), st("bm"), np.array([c["n"] for c in cases], np.int32),
                          torch.as_tensor(st("cos")).to(eng.device), torch.as_tensor(st("meta")).to(eng.device),
                          smoothing=prm[0], max_boost=prm[1], max_decay=prm[2])
    torch.cuda.synchronize()
    o = [_np(x) for x in out]
    return [(o[0][i], o[1][i], o[2][i], o[3][i], int(o[4][i]), int(o[5][i])) for i in range(len(cases))]


def test_fuse_equals_the_restatement_bit_for_bit(mods, z):
    """Every case of rerank_cases.fuse_cases (the reference's own cosines, dyadic ties, degenerate min-max, the sort's edges,
    URL groups, repeated slots, 1024 equal final scores, parameters), several queries per call."""
    eng = _engine(mods, z)
    cases = RC.fuse_cases()
    by_prm = {}
    for c in cases:
        by_prm.setdefault(c["prm"], []).append(c)
    bad = []
    for prm, cs in by_prm.items():
        for i in range(0, len(cs), 24):
            part = cs[i:i + 24]
            for c, got in zip(part, _fuse_gpu(eng, part)):
                if not RC.same_fuse(got, RC.fuse_ref(c)):
                    bad.append(c["name"])
    assert not bad, f"fuse kernel != fuse_from_gather on {bad}"


def test_fuse_on_the_reference_cosines_equals_the_fixture(mods, z):
    eng = _engine(mods, z)
    fx = RC.fixture_cases()
    got = _fuse_gpu(eng, [RC.fixture_fuse_case(f, seed=7 + i) for i, f in enumerate(fx)])
    for f, (doc, score, orig, chunk, n, rows) in zip(fx, got):
        ranked = f["stages"][-1]
        assert n == len(f["docs"]) and rows == sum(f["n_rows"])
        assert score[:n].tolist() == ranked["new_similarity"]
        exp = sorted(zip(ranked["new_similarity"], ranked["doc_id"], ranked["old_similarity"], ranked["chunk_id"]),
                     key=lambda t: (-t[0], t[1]))
        assert list(zip(score[:n].tolist(), doc[:n].tolist(), orig[:n].tolist(), [f["chunk_id"][x] for x in chunk[:n]])) == exp


def test_fuse_first_slot_of_a_repeated_document(mods, z):
    """The duplicate-slot rule on its own: documents repeated several times, a different BM25 score in every slot."""
    eng = _engine(mods, z)
    rng = np.random.default_rng(3)
    cases = RC.duplicate_slot_cases(rng) + RC.duplicate_slot_cases(rng)
    for c, got in zip(cases, _fuse_gpu(eng, cases)):
        assert RC.same_fuse(got, RC.fuse_ref(c)), c["name"]


# ------------------------------------------------------------------ gather (A)
def _expected_meta(z, cand, n, mc, d0=0, d1=None, row_base=0):
    d1 = z["N"] if d1 is None else d1
    off, grp = z["doc_off"], z["url_group"]
    Q = cand.shape[0]
    meta = np.zeros((Q, RC.M, 3), np.int32)
    live = (np.arange(RC.M)[None, :] < n[:, None]) & (cand >= d0) & (cand < d1)
    d = np.where(live, cand, 0)
    rows = np.minimum(off[d + 1] - off[d], mc)
    meta[..., 0] = np.where(live, rows, 0)
    meta[..., 1] = np.where(live, grp[d] + 2, 0)
    meta[..., 2] = np.where(live, off[d] - off[d0] + row_base, 0)
    return meta


def _check_cos(z, q_rows, cos, meta, inv_rel, tag):
    """every gathered cosine within its bar of the float64 one; slots past a candidate's rows exactly 0."""
    rows, first = meta[..., 0], meta[..., 2]
    j = np.arange(RC.MAXC)
    used = j[None, None, :] < rows[..., None]
    assert (cos[~used] == 0).all() and not np.signbit(cos[~used]).any()
    qi, mi, ji = np.nonzero(used)
    r = first[qi, mi] + ji
    c64, A = z["c64"][q_rows[qi], r], z["A"][q_rows[qi], r]
    bar = RC.gather_bar(A, c64, inv_rel[r])
    err = np.abs(cos[qi, mi, ji].astype(np.float64) - c64)
    assert (err <= bar).all(), f"{tag}: {int((err > bar).sum())} cosines outside the bar, worst {np.max(err / np.maximum(bar, 1e-300)):.3f}"
    live = bar > 0
    FRACTIONS[tag] = max(FRACTIONS.get(tag, 0.0), float(np.max(err[live] / bar[live])) if live.any() else 0.0)
    return bar, (qi, mi, ji)


def _inv_rel(eng, z, layout):
    if layout == 0:
        return np.full(z["C"], 13.0 * U32)
    inv = _np(eng._t["inv_norm"]).astype(np.float64)
    nrm = np.linalg.norm(z["emb"].astype(np.float64), axis=1)
    nrm[nrm == 0] = 1.0
    return np.abs(inv * nrm - 1.0)


def test_gather_against_float64(mods, z):
    """Both layouts x both instantiations (Q = 16: one wave per slot, Q * M = 16384; Q = 17: 8-slot waves), max_chunks
    1, 2, 9, 10: meta exact, cosines within the bar, the instantiations bit-equal within a layout and within the sum of
    their bars across layouts (only inv_norm differs)."""
    rng = np.random.default_rng(21)
    Q = 17
    qsel = np.concatenate([np.arange(8), rng.integers(0, 8, Q - 8)])
    q = z["queries"][qsel].copy()
    cand, n = RC.candidates(rng, z["N"], Q)
    n[:3] = RC.M
    n[3] = 5000
    cand[0, :7] = np.arange(7)                                              # the special documents, first and last row
    cand[1, :3] = (z["N"] - 1, 0, 6)
    got = {}
    for layout in (0, 1):
        eng = _engine(mods, z, layout)
        inv_rel = _inv_rel(eng, z, layout)
        for mc in (1, 2, 9, 10):
            c16, m16 = [_np(x) for x in eng.rerank_gather(q[:16], cand[:16], n[:16], max_chunks=mc)]
            c17, m17 = [_np(x) for x in eng.rerank_gather(q, cand, n, max_chunks=mc)]
            assert np.array_equal(_bits(c16), _bits(c17[:16])) and np.array_equal(m16, m17[:16]), (layout, mc)
            assert np.array_equal(m17, _expected_meta(z, cand, np.minimum(n, RC.M), mc)), (layout, mc)
            bar, idx = _check_cos(z, qsel, c17, m17, inv_rel, f"gather layout {layout}")
            got[layout, mc] = (c17, bar, idx)
    for mc in (1, 2, 9, 10):
        (c0, b0, i0), (c1, b1, i1) = got[0, mc], got[1, mc]
        assert (np.abs(c0[i0].astype(np.float64) - c1[i1]) <= b0 + b1).all(), mc


def test_gather_shards_and_special_queries(mods, z):
    """A shard (nonzero doc_base / row_base) gives the unsharded engine's cosines bit for bit for the documents it owns and
    zeros for the others; a zero query gives exactly 0 cosines; a NaN query leaves the other queries of the call bit-equal
    to a call without it, and its fused n is its kept-document count."""
    rng = np.random.default_rng(8)
    Q = 6
    q = z["queries"][:Q].copy()
    cand, n = RC.candidates(rng, z["N"], Q)
    whole = _engine(mods, z, 0)
    cw, mw = [_np(x) for x in whole.rerank_gather(q, cand, n, max_chunks=10)]
    d0, d1 = 400, 1100
    r0 = int(z["doc_off"][d0])
    shard = _engine(mods, z, 0, 32, d0, d1)
    cs, ms = [_np(x) for x in shard.rerank_gather(q, cand, n, doc_base=d0, row_base=r0, max_chunks=10)]
    assert np.array_equal(ms, _expected_meta(z, cand, np.minimum(n, RC.M), 10, d0, d1, r0))
    mine = (ms[..., 1] != 0)
    assert mine.any() and (~mine).any()
    assert np.array_equal(_bits(cs[mine]), _bits(cw[mine])) and np.array_equal(ms[mine], mw[mine])
    assert (_bits(cs[~mine]) == 0).all() and (ms[~mine] == 0).all()
    # zero and NaN queries
    qz = q.copy()
    qz[1] = 0.0
    qz[4] = np.nan
    cz, mz = [_np(x) for x in whole.rerank_gather(qz, cand, n, max_chunks=10)]
    assert (_bits(cz[1]) == 0).all()
    keep = [0, 1, 2, 3, 5]
    ck, mk = [_np(x) for x in whole.rerank_gather(qz[keep], cand[keep], n[keep], max_chunks=10)]
    assert np.array_equal(_bits(cz[keep]), _bits(ck)) and np.array_equal(mz, mw) and np.array_equal(mk, mw[keep])
    bm = rng.standard_normal((Q, RC.M))
    fused = [_np(x) for x in whole.rerank_fuse(cand, bm, n, torch.as_tensor(cz).to(whole.device), torch.as_tensor(mz).to(whole.device))]
    kept = rerank_ref.fuse_from_gather(cand[4], bm[4], n[4], np.zeros((RC.M, RC.MAXC), np.float32), mz[4])[4]
    assert fused[4][4] == kept and fused[5][4] == rerank_ref.fuse_from_gather(cand[4], bm[4], n[4], np.zeros((RC.M, RC.MAXC)), mz[4])[5]
    for i in keep:
        assert RC.same_fuse([x[i] for x in fused], rerank_ref.fuse_from_gather(cand[i], bm[i], n[i], cz[i], mz[i]))


# ------------------------------------------------------------------ end to end
def _explained_score_check(z, q_row, cand, bm, n, cos, meta, prm):
    """The fused list against the chain on float64 cosines (module docstring): -> the largest |score error| / sbar."""
    s, boost, decay = prm
    f32 = rerank_ref.fuse_from_gather(cand, bm, n, cos, meta, s, boost, decay, return_stages=True)
    used = np.arange(RC.MAXC)[None, :] < meta[:, 0][:, None]
    c64 = np.zeros(cos.shape)
    mi, ji = np.nonzero(used & (np.arange(RC.M) < max(0, min(n, RC.M)))[:, None])
    r = meta[mi, 2] + ji
    c64[mi, ji] = z["c64"][q_row, r]
    bar = np.zeros(cos.shape)
    bar[mi, ji] = RC.gather_bar(z["A"][q_row, r], c64[mi, ji])
    f64 = rerank_ref.fuse_from_gather(cand, bm, n, c64, meta, s, boost, decay, return_stages=True)
    n32, n64 = f32[4], f64[4]
    assert n32 == n64 and f32[5] == f64[5] and set(f32[0][:n32].tolist()) == set(f64[0][:n64].tolist())
    if n32 == 0:
        return 0.0
    docs, n_rows, st64 = f64[6]
    st32 = f32[6][2]
    # cmax - cmin of the float64 chain, bar_max over the kept rows
    slot_of = {}
    for m in range(max(0, min(n, RC.M))):
        slot_of.setdefault(int(cand[m]), m)
    kb = np.concatenate([bar[slot_of[d], :k] for d, k in zip(docs, n_rows)])
    kc = np.concatenate([c64[slot_of[d], :k] for d, k in zip(docs, n_rows)])
    rng_c = kc.max() - kc.min()
    if rng_c == 0:
        return 0.0
    sbar = (1 - s) * 2 * kb.max() / rng_c * (1 + 64 * U32) + 16 * RC.U64
    first = lambda v: int(np.flatnonzero(v == v.max())[0])
    explained, off = set(), 0
    for d, k in zip(docs, n_rows):
        b32 = np.array(st32["blend"][off:off + k]); b64 = np.array(st64["blend"][off:off + k])
        p32 = np.array(st32["positional"][off:off + k]); p64 = np.array(st64["positional"][off:off + k])
        if first(b32) != first(b64):
            assert abs(b64[first(b32)] - b64[first(b64)]) <= 2 * sbar, d
            explained.add(d)
        elif first(p32) != first(p64):
            assert abs(p64[first(p32)] - p64[first(p64)]) <= 2 * sbar, d
        off += k
    pos32 = {int(d): i for i, d in enumerate(f32[0][:n32])}
    pos64 = {int(d): i for i, d in enumerate(f64[0][:n64])}
    sc64 = {int(d): float(v) for d, v in zip(f64[0][:n64], f64[1][:n64])}
    sc32 = {int(d): float(v) for d, v in zip(f32[0][:n32], f32[1][:n32])}
    worst = 0.0
    for d in sc64:
        if d not in explained:
            e = abs(sc32[d] - sc64[d])
            assert e <= sbar, (d, e, sbar)
            worst = max(worst, e / sbar)
    ds = np.array([d for d in sc64 if d not in explained])
    if len(ds) > 1:
        a32 = np.array([pos32[d] for d in ds]); a64 = np.array([pos64[d] for d in ds]); s64 = np.array([sc64[d] for d in ds])
        inv = (np.sign(a32[:, None] - a32[None, :]) != np.sign(a64[:, None] - a64[None, :]))
        assert (np.abs(s64[:, None] - s64[None, :])[inv] <= 2 * sbar).all()
    return worst


@pytest.mark.parametrize("Q", [1, 17, 300])
def test_rerank_end_to_end(mods, z, Q):
    """DeviceEngine.rerank (max_queries = 8: slices of 128 queries) == fuse_from_gather on what rerank_gather returns for the
    same inputs, bit for bit, for max_chunks 3 and 10; and within sbar of the chain on float64 cosines."""
    eng = _engine(mods, z, 0, 8)
    rng = np.random.default_rng(100 + Q)
    qsel = rng.integers(0, len(z["queries"]), Q)
    q = z["queries"][qsel]
    cand, n = RC.candidates(rng, z["N"], Q, n_range=(1, RC.M), p_dup=0.1)
    n[rng.random(Q) < 0.2] = RC.M
    bm = rng.standard_normal((Q, RC.M)) * 20
    for mc in (3, 10):
        out = [_np(x) for x in eng.rerank(q, cand, bm, n, max_chunks=mc)]
        cos, meta = [_np(x) for x in eng.rerank_gather(q, cand, n, max_chunks=mc)]
        worst = 0.0
        for i in range(Q):
            exp = rerank_ref.fuse_from_gather(cand[i], bm[i], n[i], cos[i], meta[i])
            assert RC.same_fuse([x[i] for x in out], exp), (Q, mc, i)
            worst = max(worst, _explained_score_check(z, qsel[i], cand[i], bm[i], n[i], cos[i], meta[i], RC.DEFAULT_PRM))
        FRACTIONS["end to end score"] = max(FRACTIONS.get("end to end score", 0.0), worst)
