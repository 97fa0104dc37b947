"""Proximity search on the GPU (msr_proximity_sets, text.Near in DeviceEngine.phrase_sets, the facades): the kernel against the
oracle of proximity_ref.py on every hand-made corpus, word for word; padding, determinism, rows alone and in a batch; ordered
rows with span == L against msr_phrase_sets on the same engine; the ABI refusals; and the consumers -- BM25, dense, the
Retriever in both modes, the BM25 facade and /api/search -- bit for bit against the same call with a host-built DocSet of the
oracle's mask, asked with proximity=True text and with Near objects."""
import ctypes as C

import numpy as np
import pytest
import torch

from msretr._abi import MsrError
from msretr.docset import DeviceSets, DocSet, pack_bits
from msretr.engine import DeviceEngine
from msretr.index import CorpusIndex, _np
from msretr.index_build import bm25_index_from_token_ids
from msretr.retriever import Retriever
from msretr.text import Near
from phrase_ref import combine_mask, phrase_mask_fast
from proximity_ref import (A, B, BIG, C_, D, F, G, H, L17, VARIANTS, X, NearCase, cand_mask, corpus, expected, near_mask_fast,
                           random_rows)

pytestmark = pytest.mark.gpu
FILL = 0xA5A5A5A5
PAD = 3                                                      # words of a row behind ceil(N / 32) that must keep the fill


def _P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _i32(a, dev):
    return torch.from_numpy(np.asarray(a if len(a) else [0], np.int32)).to(dev)


def _filled(rows, words, dev):
    return torch.from_numpy(np.full((rows, words), FILL, np.uint32).view(np.int32)).to(dev)


def _host(t):
    return t.cpu().numpy().view(np.uint32)


def _cand_rows(c, dev, extra=2):
    """The corpus's candidate rows on the device: `extra` words of all-ones padding per row and every bit at or above N set."""
    N, W = c.n_docs, (c.n_docs + 31) // 32
    b = np.full((len(c.cands), W + extra), 0xFFFFFFFF, np.uint32)
    for i, (_, m) in enumerate(c.cands):
        b[i, :W] = pack_bits(m)
        if N % 32:
            b[i, W - 1] |= np.uint32((0xFFFFFFFF << (N % 32)) & 0xFFFFFFFF)
    return torch.from_numpy(b.view(np.int32)).to(dev), W + extra


def _pack(rows, dev):
    off, terms = [0], []
    for r in rows:
        terms += list(r.phrase); off.append(len(terms))
    return (_i32(off, dev), _i32(terms, dev), _i32([r.span for r in rows], dev), _i32([int(r.ordered) for r in rows], dev),
            _i32([r.cand for r in rows], dev))


def _run(eng, c, rows, with_cands=True, exact=False):
    """One msr_proximity_sets call (exact: msr_phrase_sets on the rows' phrases) into a pre-filled buffer of stride W + PAD
    -> uint32 [R, W + PAD] (host)."""
    dev = eng.device
    W = (c.n_docs + 31) // 32
    out = _filled(len(rows), W + PAD, dev)
    off, terms, span, order, rc_ = _pack(rows, dev)
    cb, cs = _cand_rows(c, dev) if with_cands else (None, 0)
    cand = (_P(cb), len(c.cands), cs, _P(rc_)) if with_cands else (_P(None), 0, 0, _P(None))
    if exact:
        rc = eng.lib.msr_phrase_sets(eng.handle, len(rows), _P(off), _P(terms), *cand, _P(out), W + PAD, eng._stream())
    else:
        rc = eng.lib.msr_proximity_sets(eng.handle, len(rows), _P(off), _P(terms), _P(span), _P(order), *cand, _P(out), W + PAD,
                                        eng._stream())
    assert rc == 0, eng.lib.msr_last_error(eng.handle)
    torch.cuda.synchronize(dev)
    return _host(out)


def _check(c, rows, want, got):
    N, W = c.n_docs, (c.n_docs + 31) // 32
    assert got.shape == (len(rows), W + PAD)
    assert (got[:, W:] == FILL).all(), "words behind ceil(N / 32) were touched"
    for i, (r, w) in enumerate(zip(rows, want)):
        assert (got[i, :W] == pack_bits(w)).all(), (N, i, r)
    if N % 32:
        assert (got[:, W - 1] >> np.uint32(N % 32) == 0).all(), "bits at or above N"


@pytest.fixture(scope="module")
def engines():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    made = {}

    def get(N, empty_ends=False):
        if (N, empty_ends) not in made:
            c = corpus(N, empty_ends)
            made[N, empty_ends] = (c, DeviceEngine(c.ix, max_queries=4, max_k=16, rerank_max_docs=0))
        return made[N, empty_ends]
    yield get
    for _, e in made.values():
        e.close()


@pytest.mark.parametrize("N,empty_ends", VARIANTS)
def test_kernel_against_the_oracle_every_case_twice(engines, N, empty_ends):
    c, eng = engines(N, empty_ends)
    assert eng.has_tokens
    rows, want = expected(N, empty_ends)
    a = _run(eng, c, rows)
    _check(c, rows, want, a)
    assert _run(eng, c, rows).tobytes() == a.tobytes()       # a second buffer: the same bytes
    # one row per call gives the same words as the row inside the batch: an exact row, both modes, every scan width
    alone = {0, len(rows) // 2, len(rows) - 7}
    for key in ("ordered: two terms over exactly", "any order: two terms over exactly", "nine terms", "five terms",
                "ordered L = 16 over exactly", "any order: first term at stream position 63"):
        alone |= {i for i, r in enumerate(rows) if r.claim.startswith(key)}
    for i in sorted(alone):
        assert (_run(eng, c, rows[i:i + 1])[0] == a[i]).all(), rows[i].claim


@pytest.mark.parametrize("N", [1025, BIG])
def test_300_random_rows_in_one_call(engines, N):
    """The oracle here is near_mask_fast, which test_proximity_cases.py holds against the plain loops on these very rows."""
    c, eng = engines(N)
    rows = random_rows(c, 300, seed=N)
    want = [near_mask_fast(c.tok_off, c.tok_ids, r.phrase, r.span, r.ordered, cand_mask(c, r.cand)) for r in rows]
    got = _run(eng, c, rows)
    _check(c, rows, want, got)
    assert _run(eng, c, rows).tobytes() == got.tobytes()
    nz = sum(int(w.any()) for w in want)
    assert 60 <= nz < 300, nz                                # the mix holds empty rows and non-empty ones
    assert {len(r.phrase) for r in rows} >= {1, 2, 3, 4} and {r.ordered for r in rows} == {True, False}


@pytest.mark.parametrize("N,empty_ends", VARIANTS)
def test_ordered_rows_with_span_L_equal_msr_phrase_sets(engines, N, empty_ends):
    c, eng = engines(N, empty_ends)
    rows = [r for r in expected(N, empty_ends)[0] if r.ordered and r.span == len(r.phrase)]
    rows += [NearCase(r.phrase, len(r.phrase), True, r.cand, r.claim) for r in random_rows(c, 60, seed=9)]
    assert len(rows) >= 80 and sum(1 for r in rows if len(r.phrase) > 8) >= 2 and sum(1 for r in rows if 4 < len(r.phrase) <= 8) >= 2
    got = _run(eng, c, rows)
    assert got.tobytes() == _run(eng, c, rows, exact=True).tobytes()
    assert got[:, :(N + 31) // 32].any()


@pytest.mark.parametrize("N", [33, BIG])
def test_no_candidate_rows_null_pointers(engines, N):
    c, eng = engines(N)
    rows = [NearCase(r.phrase, r.span, r.ordered, v, r.claim) for r in expected(N)[0][60:84] for v in (-1, 0, 9)]   # row_cand is not read
    want = [near_mask_fast(c.tok_off, c.tok_ids, r.phrase, r.span, r.ordered) for r in rows]
    _check(c, rows, want, _run(eng, c, rows, with_cands=False))
    assert any(w.any() for w in want)


def test_refusals_leave_the_outputs_untouched(engines):
    c, eng = engines(1025)
    lib, h, st, dev = eng.lib, eng.handle, eng._stream(), eng.device
    W = (c.n_docs + 31) // 32
    rows = expected(1025)[0][:4]
    p_off, p_terms, p_span, p_ord, p_cand = _pack(rows, dev)
    cb, cs = _cand_rows(c, dev)
    nc = len(c.cands)
    out = _filled(4, W, dev)
    good = dict(n=4, off=p_off, span=p_span, ord=p_ord, cb=cb, nc=nc, cs=cs, rc=p_cand, out=out, os=W)
    call = lambda a: lib.msr_proximity_sets(h, a["n"], _P(a["off"]), _P(p_terms), _P(a["span"]), _P(a["ord"]), _P(a["cb"]), a["nc"],
                                            a["cs"], _P(a["rc"]), _P(a["out"]), a["os"], st)
    for change in (dict(n=-1), dict(out=None), dict(off=None), dict(span=None), dict(ord=None), dict(os=W - 1), dict(cs=W - 1),
                   dict(nc=-1), dict(cb=None), dict(rc=None)):
        assert call(dict(good, **change)) == -1, change
        assert b"msr_proximity_sets" in lib.msr_last_error(h)
        torch.cuda.synchronize(dev)
        assert (_host(out) == FILL).all(), change
    assert lib.msr_proximity_sets(h, 0, _P(None), _P(None), _P(None), _P(None), _P(None), 0, 0, _P(None), _P(None), W, st) == 0
    assert call(dict(good, n=0)) == 0
    torch.cuda.synchronize(dev)
    assert (_host(out) == FILL).all()
    assert call(good) == 0                                   # (the arguments themselves are good)
    torch.cuda.synchronize(dev)
    assert (_host(out) != FILL).all()
    # an index without a forward index: not bound
    ix = c.ix
    plain = CorpusIndex(**{k: getattr(ix, k) for k in ("doc_ids", "doc_len", "term_off", "post_doc", "post_tf", "idf", "avgdl",
                                                       "total_docs")})
    bare = DeviceEngine(plain, max_queries=4, max_k=16, rerank_max_docs=0)
    try:
        assert not bare.has_tokens
        out.copy_(_filled(4, W, dev))
        assert bare.lib.msr_proximity_sets(bare.handle, 4, _P(p_off), _P(p_terms), _P(p_span), _P(p_ord), _P(None), 0, 0, _P(None),
                                           _P(out), W, bare._stream()) == -2
        torch.cuda.synchronize(dev)
        assert (_host(out) == FILL).all()
        with pytest.raises(MsrError, match="attach_tokens"):
            bare.phrase_sets([[Near([A, B], 2)]])
    finally:
        bare.close()


def test_engine_phrase_sets_mixes_exact_near_and_term_lists(engines):
    c, eng = engines(BIG)
    ix = c.ix
    odd = DocSet.from_mask(ix, c.cands[0][1])
    ph = lambda p: phrase_mask_fast(c.tok_off, c.tok_ids, p)
    nm = lambda p, span, ordered: near_mask_fast(c.tok_off, c.tok_ids, p, span, ordered)
    every = np.ones(BIG, bool)
    #        must                                   not                        must   must_not  within  expected mask
    Q = [([Near([A, B], 3)],                        [],                        [],    [],       None,   nm([A, B], 5, False)),
         ([Near((A, B), 3)],                        [],                        [],    [],       None,   nm([A, B], 5, False)),
         ([[A, B], Near([A, B], 3, ordered=True)],  [],                        [],    [],       None,   ph([A, B]) & nm([A, B], 5, True)),
         ([],                                       [Near([C_, D], 15)],       [],    [],       None,   ~nm([C_, D], 17, False)),
         ([Near([G, H], 62)],                       [Near([H, G], 0, True)],   [],    [3],      odd,
          nm([G, H], 64, False) & ~nm([H, G], 2, True) & ~ph([3]) & odd.mask),
         ([Near([A, -1], 2)],                       [],                        [],    [],       None,   ~every),
         ([],                                       [Near([7, -1], 1)],        [],    [],       None,   every),
         ([],                                       [],                        [X],   [],       None,   ph([X])),
         ([],                                       [],                        [],    [],       None,   every),
         ([[A, B]],                                 [],                        [],    [],       None,   ph([A, B])),
         ([Near([A, B], 3)],                        [],                        [F],   [],       odd,    nm([A, B], 5, False) & ph([F]) & odd.mask),
         ([Near([B, A, B], 1)],                     [[A, B]],                  [],    [],       None,   nm([A, B], 3, False) & ~ph([A, B]))]
    cols = list(zip(*Q))
    ds = eng.phrase_sets(list(cols[0]), list(cols[1]), list(cols[2]), list(cols[3]), within=list(cols[4]))
    assert isinstance(ds, DeviceSets) and len(ds) == len(Q)
    for q, row in enumerate(Q):
        assert ds.docset(q) == DocSet.from_mask(ix, row[5]), q
    for q in (0, 2, 3, 4, 10, 11):
        assert Q[q][5].any() and not Q[q][5].all(), q
    assert Q[2][5].sum() < Q[0][5].sum()
    # the rows against combine_mask of the oracle's masks: query 4 = AND of its must row, NOT its not row
    g = combine_mask([nm([G, H], 64, False) & ~ph([3]) & odd.mask, nm([H, G], 2, True) & odd.mask], [0], [1], BIG)
    assert ds.docset(4) == DocSet.from_mask(ix, g)
    T, P, Cn = ds.layout
    q_set = ds.q_set.cpu().tolist()
    assert q_set[8] == -1 and 0 <= q_set[7] < T
    # exact rows: A B | {A, B} (queries 2, 9 and 11 share it).  Proximity rows, behind them: A B any 5 (queries 0 and 1);  A B
    # ordered 5;  C D any 17;  G H any 64 with its query's terms and base;  H G ordered 2 inside odd;  A -1;  7 -1;  A B any 5
    # with F inside odd;  B A B any 3
    assert ds.n_near == 9 and P == 10 and Cn == 10 and ds.n_sets == T + P + Cn
    assert sorted(v for v in q_set if v >= T + P) == list(range(T + P, T + P + Cn))
    again = eng.phrase_sets(list(cols[0]), list(cols[1]), list(cols[2]), list(cols[3]), within=list(cols[4]))
    assert again.bits.cpu().numpy().tobytes() == ds.bits.cpu().numpy().tobytes()
    part = ds.queries(2, 5)
    assert part.layout == ds.layout and part.n_near == 9
    # only proximity rows: msr_phrase_sets has nothing to do
    only = eng.phrase_sets([[Near([A, B], 3)], [Near([C_, D], 0, True)]], within=odd)
    assert only.n_near == 2 and only.layout[1] == 2
    assert only.docset(0) == DocSet.from_mask(ix, nm([A, B], 5, False) & odd.mask)
    assert only.docset(1) == DocSet.from_mask(ix, ph([C_, D]) & odd.mask)
    with pytest.raises(ValueError, match="MSR_PHRASE_MAX_TERMS"):
        eng.phrase_sets([[Near(L17, 0)]])
    with pytest.raises(ValueError, match="MSR_PROX_MAX_SPAN"):
        eng.phrase_sets([[Near([A, B], 63)]])


def test_a_call_without_near_has_the_layout_it_had(engines):
    c, eng = engines(BIG)
    ph = lambda p: phrase_mask_fast(c.tok_off, c.tok_ids, p)
    ds = eng.phrase_sets([[[A, B]], [[A, B], [C_, D]], []], [[], [[G, H]], []], [[], [], [X]])
    T, P, Cn = ds.layout
    # term rows: {A, B}; {C, D}; {G, H}; {X}.  Phrase rows: A B; C D; G H.  Two queries with phrases.
    assert (T, P, Cn) == (4, 3, 2) and ds.n_near == 0 and ds.n_sets == 9
    assert ds.docset(1) == DocSet.from_mask(c.ix, ph([A, B]) & ph([C_, D]) & ~ph([G, H]))
    assert eng.term_sets([[X]], None).n_near == 0


# ------------------------------------------------------------------------------------------------ consumers
N_DOCS, V = 6007, 300
PA, PB, PC = V, V + 1, V + 2                                 # the planted terms: "alpha", "beta", "gamma"


def _word(t):
    if t == 0:
        return "tübingen"
    if t >= V:
        return ("alpha", "beta", "gamma")[t - V]
    s, t = "", int(t)
    while True:
        s = chr(ord("a") + t % 26) + s
        t //= 26
        if t == 0:
            return "w" + s


@pytest.fixture(scope="module")
def corp():
    """6007 documents of 5 .. 60 Zipf terms, built on the GPU with keep_tokens=True.  Document d holds, by d % 20: 0 alpha beta
    gamma; 1 alpha beta; 2 alpha <word> beta; 3 beta alpha; 4 alpha <word> <word> gamma; 5 beta <word> <word> <word> alpha; else
    none of the three."""
    assert torch.cuda.is_available(), "these tests need the MI355X"
    rng = np.random.default_rng(21)
    w = 1.0 / np.arange(1, V) ** 1.07
    streams = []
    for d in range(N_DOCS):
        s = (1 + rng.choice(V - 1, int(rng.integers(5, 61)), p=w / w.sum())).tolist()
        if rng.random() < 0.3:                               # the city (term 0, appended to every query): a positive idf
            s[0] = 0
        at = int(rng.integers(1, len(s) + 1))
        ins = {0: [PA, PB, PC], 1: [PA, PB], 2: [PA, 17, PB], 3: [PB, PA], 4: [PA, 17, 23, PC], 5: [PB, 17, 23, 29, PA]}.get(d % 20, [])
        streams.append(s[:at] + ins + s[at:])
    off = np.zeros(N_DOCS + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in streams])
    tok = np.asarray([t for s in streams for t in s], np.int32)
    ids = np.arange(N_DOCS, dtype=np.int64) * 2 + 100
    ix = bm25_index_from_token_ids(ids, off, tok, V + 3, device="cuda", keep_tokens=True)
    assert _np(ix.tok_off).tolist() == off.tolist() and _np(ix.tok_ids).tobytes() == tok.tobytes()
    cnt = 1 + np.arange(N_DOCS) % 3
    ix.doc_off = torch.from_numpy(np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32))
    n_chunks = int(cnt.sum())
    ix.chunk_ids = torch.arange(n_chunks, dtype=torch.int64)
    g = torch.Generator().manual_seed(5)
    emb = torch.randn((n_chunks, 768), generator=g)
    ix.emb = emb / emb.norm(dim=1, keepdim=True)
    hosts = ["uni-tuebingen.de", "tuebingen.de", "example.org"]
    ix.urls = [f"https://{hosts[d % 3]}/doc{d}" for d in range(N_DOCS)]
    ix.titles = ["" for _ in range(N_DOCS)]
    ix.texts = [" ".join(_word(t) for t in s) for s in streams]
    ix.vocab = {_word(t): t for t in range(V + 3)}
    qv = (ix.emb[rng.integers(0, n_chunks, 10)] + 0.3 * torch.randn((10, 768), generator=g)).numpy() * 7.0
    terms = [[PA, PB] + rng.integers(1, 60, 3).tolist() for _ in range(10)]
    return ix, off, tok, terms, np.ascontiguousarray(qv, np.float32)


@pytest.fixture(scope="module")
def eng(corp):
    e = DeviceEngine(corp[0], max_queries=16, max_k=1000, rerank_max_docs=1000)
    yield e
    e.close()


@pytest.fixture(scope="module")
def masks(corp):
    """The oracle's masks the consumer tests share: computed once."""
    ix, off, tok = corp[:3]
    nm = lambda p, span, ordered: near_mask_fast(off, tok, p, span, ordered, None, V + 3)
    out = {"ab_any3": nm([PA, PB], 3, False), "ab_ord3": nm([PA, PB], 3, True), "ac_ord4": nm([PA, PC], 4, True),
           "ba_any5": nm([PB, PA], 5, False), "ab_ord2": nm([PA, PB], 2, True), "w17": nm([17], 1, False), "w23": nm([23], 1, False)}
    kind = np.arange(N_DOCS) % 20
    assert out["ab_any3"][kind <= 3].all() and out["ab_ord3"][kind <= 2].all() and not out["ab_ord3"][kind == 3].all()
    assert out["ac_ord4"][(kind == 0) | (kind == 4)].all() and out["ba_any5"][(kind <= 5) & (kind != 4)].all() and not out["ab_any3"][kind == 5].all()
    return out


def _mixes(corp, masks):
    """10 queries: a must Near, a not Near, both kinds with an exact phrase, inside a site set with K11 terms, none."""
    ix = corp[0]
    site = DocSet.from_sites(ix, ["uni-tuebingen.de"])
    ab_exact = masks["ab_ord2"]
    mp, xp, m, x, within, want = [], [], [], [], [], []
    for q in range(10):
        kind = q % 6
        mp.append([Near([PA, PB], 1)] if kind in (0, 3) else [[PA, PB], Near([PA, PC], 2, ordered=True)] if kind == 2 else [])
        xp.append([Near([PA, PB], 1, ordered=True)] if kind in (1, 3) else [])
        m.append([17] if kind == 3 else [])
        x.append([23] if kind == 3 else [])
        within.append(site if kind in (3, 5) else None)
        mask = np.ones(N_DOCS, bool)
        if kind in (0, 3):
            mask &= masks["ab_any3"]
        if kind == 2:
            mask &= ab_exact & masks["ac_ord4"]
        if kind in (1, 3):
            mask &= ~masks["ab_ord3"]
        if kind == 3:
            mask &= masks["w17"] & ~masks["w23"]
        if within[q] is not None:
            mask &= within[q].mask
        want.append(None if kind == 4 else mask)
    ref = [None if mk is None else DocSet.from_mask(ix, mk) for mk in want]
    return mp, xp, m, x, within, want, ref


def _same(got, want):
    for a, b in zip(got, want):
        a, b = (a.cpu().numpy(), b.cpu().numpy()) if torch.is_tensor(a) else (a, b)
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_bm25_and_dense_topk_equal_the_host_built_sets(corp, eng, masks):
    ix, off, tok, terms, qv = corp
    mp, xp, m, x, within, want, ref = _mixes(corp, masks)
    ds = eng.phrase_sets(mp, xp, m, x, within=within)
    assert ds.n_near >= 4
    for q in range(10):
        full = DocSet.from_mask(ix, np.ones(N_DOCS, bool)) if ref[q] is None else ref[q]
        assert ds.docset(q) == full, q
    assert sum(1 for mk in want if mk is not None and mk.any()) >= 7
    for k in (100, 1000):
        got = eng.bm25_topk(terms, k=k, within=ds)
        _same(got, eng.bm25_topk(terms, k=k, within=ref))
        assert int(got[2].max()) > 0
    got = eng.dense_topk(qv, k=100, within=ds)
    _same(got, eng.dense_topk(qv, k=100, within=ref))
    doc, n = got[0].cpu().numpy(), got[3].cpu().numpy()
    for q in range(10):
        if want[q] is not None:
            assert want[q][doc[q, :n[q]]].all()


@pytest.mark.parametrize("mode", ["lexical", "hybrid"])
def test_final_lists_equal_the_host_built_sets(corp, eng, masks, mode):
    ix, off, tok, terms, qv = corp
    mp, xp, m, x, within, want, ref = _mixes(corp, masks)
    r = Retriever(indexer=eng)
    kw = dict(mode=mode, with_source=True) if mode == "hybrid" else {}
    got = r.final_lists(terms, qv, 1000, within=within, must=m, must_not=x, must_phrases=mp, must_not_phrases=xp, **kw)
    ref_lists = r.final_lists(terms, qv, 1000, within=ref, **kw)
    _same(got, ref_lists)
    assert int(got[3].max()) > 0
    for q in range(10):
        if want[q] is not None:
            assert want[q][got[0][q, :got[3][q]]].all()
    # term strings instead of ids, and chunks of 4 queries: one phrase_sets call per chunk
    words = lambda lists: [[p.with_terms([_word(t) for t in p.terms]) if isinstance(p, Near) else [_word(t) for t in p] for p in ps]
                           for ps in lists]
    _same(r.final_lists(terms, qv, 1000, chunk=4, within=within, must=m, must_not=x, must_phrases=words(mp),
                        must_not_phrases=words(xp), **kw), ref_lists)
    with pytest.raises(ValueError, match="parse_proximity"):
        r.final_lists(terms, qv, 1000, proximity=True)


def _docs(rows):
    return [(int(row["doc_id"]) - 100) // 2 for row in rows]


def test_retriever_and_bm25_facades(corp, eng, masks):
    ix, off, tok, terms, qv = corp
    r = Retriever(indexer=eng)
    e0 = qv[0]
    within = lambda name, neg=False: DocSet.from_mask(ix, ~masks[name] if neg else masks[name])
    for mode in ("lexical", "hybrid"):
        kw = dict(query_embedding=e0, mode=mode)
        got = r.search('"alpha beta"~1', proximity=True, **kw)
        assert got and got == r.search("alpha beta", within=within("ab_any3"), **kw)
        assert masks["ab_any3"][_docs(got)].all()            # only pages with the words within three tokens ...
        exact = r.search('"alpha beta"', phrases=True, **kw)
        assert set(_docs(got)) - set(_docs(exact))           # ... among them pages the exact phrase loses
        assert got == r.search("alpha beta", must_phrases=[Near("alpha beta", 1)], **kw)
        assert got == r.search("alpha beta", must_phrases=[Near(["beta", "alpha"], 1)], **kw)
        ordered = r.search('"alpha beta"~>1', proximity=True, **kw)
        assert ordered and ordered == r.search("alpha beta", within=within("ab_ord3"), **kw) and ordered != got
        assert ordered == r.search("alpha beta", must_phrases=[Near("alpha beta", 1, ordered=True)], **kw)
        # without a suffix proximity=True is phrases=True
        assert r.search('"alpha beta" -"beta alpha"', proximity=True, **kw) == r.search('"alpha beta" -"beta alpha"', phrases=True, **kw)
        neg = r.search('alpha -"alpha beta"~>1', proximity=True, **kw)
        assert neg and not masks["ab_ord3"][_docs(neg)].any()
        assert neg == r.search("alpha", within=within("ab_ord3", neg=True), **kw)
        assert neg == r.search("alpha", must_not_phrases=[Near(["alpha", "beta"], 1, ordered=True)], **kw)
        assert r.search('"alpha unknownword"~5', proximity=True, **kw) == []
        # proximity off: the suffix is what it was -- punctuation
        text = '"alpha beta"~1'
        assert r.search(text, phrases=True, **kw) == r.search('"alpha beta"', phrases=True, **kw)
        assert r.search(text, proximity=False, **kw) == r.search(text, **kw)
        # a proximity condition, an exact phrase, operators and a site set together
        site = DocSet.from_sites(ix, ["uni-tuebingen.de"])
        both = r.search(f'"beta alpha"~3 "alpha gamma"~>2 -{_word(23)}', proximity=True, operators=True, within=site, **kw)
        keep = masks["ba_any5"] & masks["ac_ord4"] & ~masks["w23"] & site.mask
        assert both and both == r.search("beta alpha alpha gamma", within=DocSet.from_mask(ix, keep), **kw)
    # batch: per-query conditions, one of them without
    qs = ['"alpha gamma"~>2', "alpha beta", 'beta -"alpha beta"~>1']
    got = r.search_batch(qs, query_embeddings=qv[:3], proximity=True)
    assert got[0] == r.search("alpha gamma", within=within("ac_ord4"), query_embedding=qv[0])
    assert got[1] == r.search("alpha beta", query_embedding=qv[1])
    lines = r.batch_search(list(zip("123", qs)), query_embeddings=qv[:3], proximity=True)
    assert [e["url"] for e in lines if e["query_num"] == "3"][:100] == [d["url"] for d in got[2]]
    with pytest.raises(ValueError, match="MSR_PHRASE_MAX_TERMS"):
        r.search("alpha", must_phrases=[Near(" ".join(["alpha"] * 17), 1)], query_embedding=e0)
    with pytest.raises(ValueError, match="MSR_PROX_MAX_SPAN"):
        r.search('"alpha beta"~63', proximity=True, query_embedding=e0)
    # the BM25 facade (its query is taken as it is: no city)
    bm = r.bm25.search('"alpha beta"~1 -"alpha gamma"~>2', top_k=50, proximity=True)
    assert bm and bm == r.bm25.search("alpha beta", top_k=50, within=DocSet.from_mask(ix, masks["ab_any3"] & ~masks["ac_ord4"]))
    assert bm == r.bm25.search("alpha beta", top_k=50, must_phrases=[Near("alpha beta", 1)],
                               must_not_phrases=[Near(["alpha", "gamma"], 2, ordered=True)])
    assert r.bm25.search('"alpha unknownword"~2', proximity=True) == []


def test_http_search_with_proximity(corp, eng, masks):
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from msretr.server import create_app
    ix, off, tok, terms, qv = corp
    r = Retriever(indexer=eng)
    client = TestClient(create_app(r))
    body = {"query": '"alpha beta"~1 -"alpha gamma"~>2', "top_k": 1000, "query_id": "q1", "query_embedding": qv[0].tolist()}
    plain = client.post("/api/search", json=body)
    prox = client.post("/api/search", json=dict(body, proximity=True))
    assert plain.status_code == 200 and prox.status_code == 200
    want = r.search(body["query"], top_k=1000, query_embedding=qv[0], query_id="q1", proximity=True)
    assert prox.json()["documents"] == want and want
    keep = DocSet.from_mask(ix, masks["ab_any3"] & ~masks["ac_ord4"])
    assert want == r.search("alpha beta", top_k=1000, query_embedding=qv[0], query_id="q1", within=keep)
    assert plain.json()["documents"] == r.search(body["query"], top_k=1000, query_embedding=qv[0], query_id="q1")
    assert plain.json()["documents"] != want
    lists = client.post("/api/search", json=dict(body, query="alpha beta", mode="hybrid", must_phrases=[{"phrase": "alpha beta", "slop": 1}],
                                                 must_not_phrases=[{"phrase": "alpha gamma", "slop": 2, "ordered": True}, "beta alpha"]))
    assert lists.status_code == 200
    assert lists.json()["documents"] == r.search("alpha beta", top_k=1000, query_embedding=qv[0], query_id="q1", mode="hybrid",
                                                 must_phrases=[Near("alpha beta", 1)],
                                                 must_not_phrases=[Near("alpha gamma", 2, ordered=True), "beta alpha"])
    assert lists.json()["documents"]
    # what the facade refuses with ValueError is the caller's error
    for bad in (dict(must_phrases=[{"phrase": "alpha beta", "slop": -1}]), dict(must_phrases=[{"phrase": "alpha beta", "slop": 63}]),
                dict(query='"alpha beta"~70', proximity=True), dict(must_not_phrases=[{"phrase": " ".join(["alpha"] * 17)}])):
        resp = client.post("/api/search", json=dict(dict(body, query="alpha beta"), **bad))
        assert resp.status_code == 400 and resp.json()["error"], bad
