"""Phrase search on the GPU (msr_bind_tokens, msr_phrase_sets, msr_combine_sets, DeviceEngine.phrase_sets, the facades): the
kernel against the oracle of phrase_ref.py on every hand-made corpus, word for word; padding, determinism, rows alone and in
a batch; the combine kernel; the ABI refusals; and the consumers -- BM25, dense, the rerank chain in both modes, the Retriever /
BM25 facades and /api/search -- bit for bit against the same call with a host-built DocSet of the oracle's mask."""
import ctypes as C

import numpy as np
import pytest
import torch

from msretr._abi import MsrError
from msretr.docset import DeviceSets, DocSet, pack_bits
from msretr.engine import DeviceEngine
from msretr.index import CorpusIndex, _np
from msretr.index_build import bm25_add_token_ids, bm25_index_from_token_ids, remove_documents
from msretr.retriever import Retriever
from phrase_ref import (A, B, BIG, C_, D, E, G, H, L17, N_TERMS, X, Y, RowCase, cand_mask, combine_mask, corpus, expected,
                        phrase_mask_fast, random_rows)

pytestmark = pytest.mark.gpu
FILL = 0xA5A5A5A5
PAD = 3                                                      # words of a row behind ceil(N / 32) that must keep the fill
VARIANTS = [(1, False), (33, False), (33, True), (1025, False), (1025, True), (8193, False), (BIG, False)]


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
    return _i32(off, dev), _i32(terms, dev), _i32([r.cand for r in rows], dev)


def _run(eng, c, rows, with_cands=True):
    """One msr_phrase_sets call into a pre-filled buffer of stride W + PAD -> uint32 [R, W + PAD] (host)."""
    dev = eng.device
    W = (c.n_docs + 31) // 32
    out = _filled(len(rows), W + PAD, dev)
    off, terms, rc_ = _pack(rows, dev)
    if with_cands:
        cb, cs = _cand_rows(c, dev)
        rc = eng.lib.msr_phrase_sets(eng.handle, len(rows), _P(off), _P(terms), _P(cb), len(c.cands), cs, _P(rc_), _P(out),
                                     W + PAD, eng._stream())
    else:
        rc = eng.lib.msr_phrase_sets(eng.handle, len(rows), _P(off), _P(terms), _P(None), 0, 0, _P(None), _P(out), W + PAD,
                                     eng._stream())
    assert rc == 0, eng.lib.msr_last_error(eng.handle)
    torch.cuda.synchronize(dev)
    return _host(out)


def _check(c, rows, want, got):
    N, W = c.n_docs, (c.n_docs + 31) // 32
    assert got.shape == (len(rows), W + PAD)
    assert (got[:, W:] == FILL).all(), "words behind ceil(N / 32) were touched"
    for i, (r, w) in enumerate(zip(rows, want)):
        assert (got[i, :W] == pack_bits(w)).all(), (N, i, r.claim)
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
    for i in (0, len(rows) // 2, len(rows) - 7):             # one row per call gives the same words as the row inside the batch
        assert (_run(eng, c, rows[i:i + 1])[0] == a[i]).all(), rows[i].claim


@pytest.mark.parametrize("N", [1025, BIG])
def test_300_random_rows_in_one_call(engines, N):
    """The oracle here is phrase_mask_fast, which test_phrase_cases.py holds against the plain loop on every case."""
    c, eng = engines(N)
    rows = random_rows(c, 300, seed=N)
    want = [phrase_mask_fast(c.tok_off, c.tok_ids, r.phrase, cand_mask(c, r.cand)) for r in rows]
    got = _run(eng, c, rows)
    _check(c, rows, want, got)
    assert _run(eng, c, rows).tobytes() == got.tobytes()
    nz = sum(int(w.any()) for w in want)
    assert 60 <= nz < 300, nz                                # the mix holds empty rows and non-empty ones


@pytest.mark.parametrize("N", [33, BIG])
def test_no_candidate_rows_null_pointers(engines, N):
    c, eng = engines(N)
    rows = [RowCase(r.phrase, v, r.claim) for r in expected(N)[0][:24] for v in (-1, 0, 9)]          # row_cand is not read
    want = [phrase_mask_fast(c.tok_off, c.tok_ids, r.phrase) for r in rows]
    _check(c, rows, want, _run(eng, c, rows, with_cands=False))


def _combine(eng, N, in_bits, n_in, in_stride, lists, out=None, out_stride=None):
    dev = eng.device
    W = (N + 31) // 32
    a_off, a, x_off, x = [0], [], [0], []
    for ands, nots in lists:
        a += ands; a_off.append(len(a))
        x += nots; x_off.append(len(x))
    out = _filled(len(lists), W + PAD, dev) if out is None else out
    d_aoff, d_a, d_xoff, d_x = _i32(a_off, dev), _i32(a, dev), _i32(x_off, dev), _i32(x, dev)    # (alive until the call has run)
    rc = eng.lib.msr_combine_sets(eng.handle, len(lists), _P(d_aoff), _P(d_a), _P(d_xoff), _P(d_x), _P(in_bits), n_in, in_stride,
                                  _P(out), out_stride or W + PAD, eng._stream())
    torch.cuda.synchronize(dev)
    return rc, _host(out)


@pytest.mark.parametrize("N", [1, 33, 1025, BIG])
def test_combine_sets_against_combine_mask(engines, N):
    c, eng = engines(N)
    rng = np.random.default_rng(N)
    W, n_in = (N + 31) // 32, 5
    masks = [rng.random(N) < p for p in (0.5, 0.9, 0.1, 0.5, 1.1)]
    host = np.full((n_in, W + 2), 0xFFFFFFFF, np.uint32)     # padding words and the bits at or above N are set
    for i, m in enumerate(masks):
        host[i, :W] = pack_bits(m)
        if N % 32:
            host[i, W - 1] |= np.uint32((0xFFFFFFFF << (N % 32)) & 0xFFFFFFFF)
    dev_in = torch.from_numpy(host.view(np.int32)).to(eng.device)
    lists = [([], []), ([0], []), ([0, 1], [2]), ([], [0, 3]), ([4], [2, 2]), ([0, 5], []), ([-1], []), ([1], [-1, 5, 99]),
             ([0, 1, 3, 4], [2]), ([4], [4]), ([1, 1], [])]
    lists += [(rng.integers(-1, 7, rng.integers(0, 4)).tolist(), rng.integers(-1, 7, rng.integers(0, 4)).tolist()) for _ in range(40)]
    rc, got = _combine(eng, N, dev_in, n_in, W + 2, lists)
    assert rc == 0, eng.lib.msr_last_error(eng.handle)
    assert (got[:, W:] == FILL).all()
    for i, (ands, nots) in enumerate(lists):
        assert (got[i, :W] == pack_bits(combine_mask(masks, ands, nots, N))).all(), (N, i, ands, nots)
    assert _combine(eng, N, dev_in, n_in, W + 2, lists)[1].tobytes() == got.tobytes()
    # no input rows at all: every AND index is out of range, NULL in_bits is not read
    rc, got = _combine(eng, N, None, 0, 0, [([], []), ([0], []), ([], [0])])
    assert rc == 0
    full = pack_bits(np.ones(N, bool))
    assert (got[0, :W] == full).all() and not got[1, :W].any() and (got[2, :W] == full).all()


def test_bind_tokens_refuses_malformed_streams():
    c = corpus(33)
    eng = DeviceEngine(c.ix, max_queries=4, max_k=16, rerank_max_docs=0)
    try:
        lib, h, st, dev = eng.lib, eng.handle, eng._stream(), eng.device
        N, T = c.n_docs, len(c.tok_ids)
        off, tok = torch.from_numpy(c.tok_off).to(dev), torch.from_numpy(c.tok_ids).to(dev)
        desc = c.tok_off.copy(); desc[7] = desc[6] - 1
        big = c.tok_ids.copy(); big[T // 2] = N_TERMS
        neg = c.tok_ids.copy(); neg[0] = -1
        start = c.tok_off.copy(); start[0] = 1
        dv = lambda a: torch.from_numpy(a).to(dev)
        W = (N + 31) // 32
        rows = expected(33)[0][:3]
        p_off, p_terms, _ = _pack(rows, dev)
        out = _filled(3, W, dev)
        phrase = lambda: lib.msr_phrase_sets(h, 3, _P(p_off), _P(p_terms), _P(None), 0, 0, _P(None), _P(out), W, st)
        assert phrase() == 0
        for o, t, n_docs, n_tok, why in ((dv(desc), tok, N, T, b"descends"), (off, tok, N, T - 1, b"from 0 to n_tokens"),
                                         (dv(start), tok, N, T, b"from 0 to n_tokens"), (off, dv(big), N, T, b"token id"),
                                         (off, dv(neg), N, T, b"token id"), (off, tok, N - 1, T, b"n_docs"),
                                         (None, tok, N, T, b"bad argument"), (off, None, N, T, b"bad argument"),
                                         (off, tok, N, -1, b"bad argument")):
            assert lib.msr_bind_tokens(h, _P(o), _P(t), n_docs, n_tok, st) == -1, why
            assert why in lib.msr_last_error(h), (why, lib.msr_last_error(h))
            out.copy_(_filled(3, W, dev))
            assert phrase() == -2                            # a refused bind leaves no binding: nothing malformed is scanned
            torch.cuda.synchronize(dev)
            assert (_host(out) == FILL).all()
        assert lib.msr_bind_tokens(h, _P(off), _P(tok), N, T, st) == 0
        assert phrase() == 0
        torch.cuda.synchronize(dev)
        for i, r in enumerate(rows):                         # (no candidate rows in this call: every document)
            assert (_host(out)[i] == pack_bits(phrase_mask_fast(c.tok_off, c.tok_ids, r.phrase))).all()
        # msr_bind_postings drops the tokens (they describe the old documents), and so does msr_unbind
        eng.rebind(c.ix)
        assert eng.has_tokens and phrase() == 0
        t = eng._t
        assert lib.msr_bind_postings(h, _P(t["term_off"]), c.ix.n_terms, _P(t["post_doc"]), _P(t["post_tf"]), int(t["post_doc"].numel()),
                                     _P(t["doc_len"]), N, _P(t["idf"]), C.c_float(c.ix.avgdl), C.c_double(c.ix.k1),
                                     C.c_double(c.ix.b), st) == 0
        assert phrase() == -2
        assert lib.msr_bind_tokens(h, _P(off), _P(tok), N, T, st) == 0 and phrase() == 0
        torch.cuda.synchronize(dev)
        assert lib.msr_unbind(h) == 0
        out.copy_(_filled(3, W, dev))
        assert phrase() == -2
        torch.cuda.synchronize(dev)
        assert (_host(out) == FILL).all()
    finally:
        eng.close()
    # without postings there is nothing to bind to
    bare = DeviceEngine(CorpusIndex(doc_ids=np.arange(5, dtype=np.int64)), max_queries=4, max_k=16, rerank_max_docs=0)
    try:
        z = torch.zeros(6, dtype=torch.int64, device=bare.device)
        assert bare.lib.msr_bind_tokens(bare.handle, _P(z), _P(None), 5, 0, bare._stream()) == -2
        assert not bare.has_tokens
    finally:
        bare.close()


def test_refusals_leave_the_outputs_untouched(engines):
    c, eng = engines(1025)
    lib, h, st, dev = eng.lib, eng.handle, eng._stream(), eng.device
    W = (c.n_docs + 31) // 32
    rows = expected(1025)[0][:4]
    p_off, p_terms, p_cand = _pack(rows, dev)
    cb, cs = _cand_rows(c, dev)
    nc = len(c.cands)
    out = _filled(4, W, dev)
    good = dict(n=4, off=p_off, cb=cb, nc=nc, cs=cs, rc=p_cand, out=out, os=W)
    for change in (dict(n=-1), dict(out=None), dict(off=None), dict(os=W - 1), dict(cs=W - 1), dict(nc=-1), dict(cb=None),
                   dict(rc=None)):
        a = dict(good, **change)
        rc = lib.msr_phrase_sets(h, a["n"], _P(a["off"]), _P(p_terms), _P(a["cb"]), a["nc"], a["cs"], _P(a["rc"]), _P(a["out"]),
                                 a["os"], st)
        assert rc == -1, change
        assert b"msr_phrase_sets" in lib.msr_last_error(h)
        torch.cuda.synchronize(dev)
        assert (_host(out) == FILL).all(), change
    assert lib.msr_phrase_sets(h, 0, _P(None), _P(None), _P(None), 0, 0, _P(None), _P(None), W, st) == 0
    assert lib.msr_phrase_sets(h, 0, _P(p_off), _P(p_terms), _P(cb), nc, cs, _P(p_cand), _P(out), W, st) == 0
    # msr_combine_sets
    lists = [([0], [1])] * 4
    for os_, n_in, in_bits, in_stride in ((W - 1, nc, cb, cs), (W, -1, cb, cs), (W, nc, None, cs), (W, nc, cb, W - 1)):
        rc, got = _combine(eng, c.n_docs, in_bits, n_in, in_stride, lists, out=out, out_stride=os_)
        assert rc == -1 and b"msr_combine_sets" in lib.msr_last_error(h)
        assert (got == FILL).all()
    z = _i32([0, 0, 0, 0, 0], dev)
    assert lib.msr_combine_sets(h, -1, _P(z), _P(z), _P(z), _P(z), _P(cb), nc, cs, _P(out), W, st) == -1
    assert lib.msr_combine_sets(h, 4, _P(None), _P(z), _P(z), _P(z), _P(cb), nc, cs, _P(out), W, st) == -1
    assert lib.msr_combine_sets(h, 4, _P(z), _P(z), _P(None), _P(z), _P(cb), nc, cs, _P(out), W, st) == -1
    assert lib.msr_combine_sets(h, 4, _P(z), _P(z), _P(z), _P(z), _P(cb), nc, cs, _P(None), W, st) == -1
    assert lib.msr_combine_sets(h, 0, _P(None), _P(None), _P(None), _P(None), _P(None), 0, 0, _P(None), W, st) == 0
    torch.cuda.synchronize(dev)
    assert (_host(out) == FILL).all()
    # an index without a forward index: not bound
    ix = c.ix
    plain = CorpusIndex(**{k: getattr(ix, k) for k in ("doc_ids", "doc_len", "term_off", "post_doc", "post_tf", "idf", "avgdl",
                                                       "total_docs")})
    bare = DeviceEngine(plain, max_queries=4, max_k=16, rerank_max_docs=0)
    try:
        assert not bare.has_tokens
        assert bare.lib.msr_phrase_sets(bare.handle, 4, _P(p_off), _P(p_terms), _P(None), 0, 0, _P(None), _P(out), W,
                                        bare._stream()) == -2
        torch.cuda.synchronize(dev)
        assert (_host(out) == FILL).all()
        with pytest.raises(MsrError, match="attach_tokens"):
            bare.phrase_sets([[[A, B]]])
    finally:
        bare.close()


def _term(c, t):
    return phrase_mask_fast(c.tok_off, c.tok_ids, [t])


def test_engine_phrase_sets_mixes_dedup_and_docset(engines):
    c, eng = engines(BIG)
    ix = c.ix
    odd = DocSet.from_mask(ix, c.cands[0][1])
    ph = lambda p, m=None: phrase_mask_fast(c.tok_off, c.tok_ids, p, m)
    every = np.ones(BIG, bool)
    #        must phrases          not phrases   must   must_not  within   expected mask
    Q = [([[A, B]],                [],           [],    [],       None,    ph([A, B])),
         ([[A, B]],                [],           [],    [],       None,    ph([A, B])),
         ([[A, B], [C_, D]],       [],           [],    [],       None,    ph([A, B]) & ph([C_, D])),
         ([],                      [[A, B]],     [],    [],       None,    ~ph([A, B])),
         ([],                      [],           [X],   [],       None,    _term(c, X)),
         ([],                      [],           [],    [],       None,    every),
         ([[A, B]],                [],           [],    [],       odd,     ph([A, B]) & odd.mask),
         ([[A, B]],                [],           [X],   [],       None,    ph([A, B]) & _term(c, X)),
         ([],                      [[X, Y]],     [],    [],       odd,     odd.mask & ~ph([X, Y])),
         ([[A, -1]],               [],           [],    [],       None,    ~every),
         ([[]],                    [],           [],    [],       None,    ~every),
         ([[G, H]],                [[H, G], [G, H, E]], [], [3],  None,    ph([G, H]) & ~ph([H, G]) & ~ph([G, H, E]) & ~_term(c, 3)),
         ([],                      [[7, -1], []], [],   [],       None,    every),
         ([],                      [],           [],    [],       odd,     odd.mask),
         ([[5, 9]],                [[9, 5]],     [],    [X],      odd,     ph([5, 9]) & ~ph([9, 5]) & ~_term(c, X) & odd.mask)]
    cols = list(zip(*Q))
    ds = eng.phrase_sets(list(cols[0]), list(cols[1]), list(cols[2]), list(cols[3]), within=list(cols[4]))
    assert isinstance(ds, DeviceSets) and len(ds) == len(Q)
    for q, row in enumerate(Q):
        assert ds.docset(q) == DocSet.from_mask(ix, row[5]), q
    assert Q[0][5].any() and Q[2][5].sum() < Q[0][5].sum() and Q[11][5].any()
    q_set = ds.q_set.cpu().tolist()
    T, P, Cn = ds.layout
    assert q_set[5] == -1 and 0 <= q_set[4] < T and 0 <= q_set[13] < T          # no phrases: the K11 row, -1, or the base's row
    assert ds.docset(13) == odd
    # distinct (phrase, candidate row) pairs: A B | {A, B};  C D;  A B inside odd;  A B with X;  X Y inside odd;  A -1;  the
    # empty phrase;  G H;  H G;  G H E;  7 -1;  5 9 with its query's terms and base;  9 5 with the base alone
    # (queries 0, 1, 2 and 3 share the first one, queries 10 and 12 the empty phrase)
    assert P == 13 and Cn == 12 and ds.n_sets == T + P + Cn
    assert sorted(v for v in q_set if v >= T + P) == list(range(T + P, T + P + Cn))
    bits, q2, n_sets, stride = eng.pack_within(ds, len(Q))                      # handed on unchanged
    assert bits is ds.bits and q2 is ds.q_set and (n_sets, stride) == (ds.n_sets, ds.stride)
    again = eng.phrase_sets(list(cols[0]), list(cols[1]), list(cols[2]), list(cols[3]), within=list(cols[4]))
    assert again.bits.cpu().numpy().tobytes() == ds.bits.cpu().numpy().tobytes()
    # one DocSet for every query; must_phrases alone
    ds2 = eng.phrase_sets([[[A, B]], [[C_, D, E]]], within=odd)
    assert ds2.docset(0) == DocSet.from_mask(ix, ph([A, B]) & odd.mask) and ds2.docset(1) == DocSet.from_mask(ix, ph([C_, D, E]) & odd.mask)
    with pytest.raises(ValueError, match="MSR_PHRASE_MAX_TERMS"):
        eng.phrase_sets([[L17]])
    with pytest.raises(ValueError):
        eng.phrase_sets([[[A, B]]], [[], []])
    with pytest.raises(TypeError):
        eng.phrase_sets([[[A, B]]] * len(Q), within=ds)


# ------------------------------------------------------------------------------------------------ consumers
N_DOCS, V = 6007, 300
PA, PB, PC = V, V + 1, V + 2                                 # the planted phrase's terms: "alpha beta gamma"


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
    gamma; 1 alpha beta; 2 alpha <word> beta; 3 beta alpha; 4 alpha .. gamma apart; else none of the three (so every word of
    a query has a positive idf: alpha is in a quarter of the documents, the city in 30 %)."""
    assert torch.cuda.is_available(), "these tests need the MI355X"
    rng = np.random.default_rng(21)
    w = 1.0 / np.arange(1, V) ** 1.07
    streams = []
    for d in range(N_DOCS):
        s = (1 + rng.choice(V - 1, int(rng.integers(5, 61)), p=w / w.sum())).tolist()
        if rng.random() < 0.3:                               # the city (term 0, appended to every query): a positive idf
            s[0] = 0
        at = int(rng.integers(1, len(s) + 1))
        ins = {0: [PA, PB, PC], 1: [PA, PB], 2: [PA, 17, PB], 3: [PB, PA], 4: [PA, 17, 23, PC]}.get(d % 20, [])
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


def _mixes(corp):
    """10 queries: a must phrase, a not phrase, both, both inside a site set with K11 terms, none, none inside a site set."""
    ix, off, tok = corp[:3]
    ph = lambda p: phrase_mask_fast(off, tok, p, None, V + 3)
    site = DocSet.from_sites(ix, ["uni-tuebingen.de"])
    mp, xp, m, x, within, masks = [], [], [], [], [], []
    for q in range(10):
        kind = q % 6
        mp.append([[PA, PB]] if kind in (0, 2, 3) else [])
        xp.append([[PB, PA]] if kind == 1 else [[PA, PB, PC]] if kind == 2 else [[PB, PC], [PB, PA]] if kind == 3 else [])
        m.append([17] if kind == 3 else [])
        x.append([23] if kind == 3 else [])
        within.append(site if kind in (3, 5) else None)
        mask = np.ones(N_DOCS, bool)
        for p in mp[q]:
            mask &= ph(p)
        for p in xp[q]:
            mask &= ~ph(p)
        for t in m[q]:
            mask &= ph([t])
        for t in x[q]:
            mask &= ~ph([t])
        if within[q] is not None:
            mask &= within[q].mask
        plain = not (mp[q] or xp[q] or m[q] or x[q] or within[q] is not None)
        masks.append(None if plain else mask)
    ref = [None if mk is None else DocSet.from_mask(ix, mk) for mk in masks]
    return mp, xp, m, x, within, masks, ref


def _same(got, want):
    for a, b in zip(got, want):
        a, b = (a.cpu().numpy(), b.cpu().numpy()) if torch.is_tensor(a) else (a, b)
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_bm25_and_dense_topk_equal_the_host_built_sets(corp, eng):
    ix, off, tok, terms, qv = corp
    mp, xp, m, x, within, masks, ref = _mixes(corp)
    ds = eng.phrase_sets(mp, xp, m, x, within=within)
    for q in range(10):
        want = DocSet.from_mask(ix, np.ones(N_DOCS, bool)) if ref[q] is None else ref[q]
        assert ds.docset(q) == want, q
    assert sum(1 for mk in masks if mk is not None and mk.any()) >= 7
    for k in (100, 1000):
        got = eng.bm25_topk(terms, k=k, within=ds)
        _same(got, eng.bm25_topk(terms, k=k, within=ref))
        assert int(got[2].max()) > 0
    got = eng.dense_topk(qv, k=100, within=ds)
    _same(got, eng.dense_topk(qv, k=100, within=ref))
    doc, n = got[0].cpu().numpy(), got[3].cpu().numpy()
    for q in range(10):
        if masks[q] is not None:
            assert masks[q][doc[q, :n[q]]].all()


@pytest.mark.parametrize("mode", ["lexical", "hybrid"])
def test_final_lists_equal_the_host_built_sets(corp, eng, mode):
    ix, off, tok, terms, qv = corp
    mp, xp, m, x, within, masks, ref = _mixes(corp)
    r = Retriever(indexer=eng)
    kw = dict(mode=mode, with_source=True) if mode == "hybrid" else {}
    got = r.final_lists(terms, qv, 1000, within=within, must=m, must_not=x, must_phrases=mp, must_not_phrases=xp, **kw)
    want = r.final_lists(terms, qv, 1000, within=ref, **kw)
    _same(got, want)
    assert len(got) == (5 if mode == "hybrid" else 4) and int(got[3].max()) > 0
    for q in range(10):
        if masks[q] is not None:
            assert masks[q][got[0][q, :got[3][q]]].all()
    # term strings instead of ids, and chunks of 4 queries: one phrase_sets call per chunk
    words = lambda lists: [[[_word(t) for t in p] for p in ps] for ps in lists]
    _same(r.final_lists(terms, qv, 1000, chunk=4, within=within, must=m, must_not=x, must_phrases=words(mp),
                        must_not_phrases=words(xp), **kw), want)
    with pytest.raises(ValueError):
        r.final_lists(terms, qv, 1000, phrases=True)
    with pytest.raises(ValueError):
        r.final_lists(terms, qv, 1000, must_phrases=mp[:3])
    with pytest.raises(ValueError, match="MSR_PHRASE_MAX_TERMS"):
        r.final_lists(terms[:1], qv[:1], 1000, must_phrases=[[list(range(17))]])


def _docs(rows):
    return [(int(row["doc_id"]) - 100) // 2 for row in rows]


def test_retriever_and_bm25_facades(corp, eng):
    ix, off, tok, terms, qv = corp
    r = Retriever(indexer=eng)
    ph = lambda p: phrase_mask_fast(off, tok, p, None, V + 3)
    ab, abc, ba = ph([PA, PB]), ph([PA, PB, PC]), ph([PB, PA])
    e0 = qv[0]
    for mode in ("lexical", "hybrid"):
        got = r.search('"alpha beta"', phrases=True, query_embedding=e0, mode=mode)
        assert got and got == r.search("alpha beta", within=DocSet.from_mask(ix, ab), query_embedding=e0, mode=mode)
        assert ab[_docs(got)].all()                          # only pages with the phrase ...
        plain = r.search("alpha beta", query_embedding=e0, mode=mode)
        apart = [d for d in _docs(plain) if not ab[d]]
        assert apart and not set(apart) & set(_docs(got))    # ... and the pages that hold the words apart are gone
        assert got == r.search("alpha beta", must_phrases=["alpha beta"], query_embedding=e0, mode=mode)
        assert got == r.search("alpha beta", must_phrases=[["alpha", "beta"]], query_embedding=e0, mode=mode)
        neg = r.search('alpha -"alpha beta gamma"', phrases=True, query_embedding=e0, mode=mode)
        assert neg and not abc[_docs(neg)].any()
        assert neg == r.search("alpha", within=DocSet.from_mask(ix, ~abc), query_embedding=e0, mode=mode)
        assert r.search('"alpha unknownword"', phrases=True, query_embedding=e0, mode=mode) == []
        # phrases off: the quotes are what they were -- punctuation
        text = '"alpha beta" -"beta alpha"'
        assert r.search(text, phrases=False, query_embedding=e0, mode=mode) == r.search(text, query_embedding=e0, mode=mode)
        # phrases, operators and a site set together
        site = DocSet.from_sites(ix, ["uni-tuebingen.de"])
        both = r.search(f'"alpha beta" -"beta alpha" -{_word(23)}', phrases=True, operators=True, within=site, query_embedding=e0,
                        mode=mode)
        keep = ab & ~ba & ~ph([23]) & site.mask
        assert both and both == r.search("alpha beta", within=DocSet.from_mask(ix, keep), query_embedding=e0, mode=mode)
    # batch: per-query phrases, one of them without
    qs = ['"alpha beta gamma"', "alpha beta", 'beta -"beta alpha"']
    got = r.search_batch(qs, query_embeddings=qv[:3], phrases=True)
    assert got[0] == r.search("alpha beta gamma", within=DocSet.from_mask(ix, abc), query_embedding=qv[0])
    assert got[1] == r.search("alpha beta", query_embedding=qv[1])
    lines = r.batch_search(list(zip("123", qs)), query_embeddings=qv[:3], phrases=True)
    assert [e["url"] for e in lines if e["query_num"] == "3"][:100] == [d["url"] for d in got[2]]
    with pytest.raises(ValueError, match="MSR_PHRASE_MAX_TERMS"):
        r.search("alpha", must_phrases=[" ".join(["alpha"] * 17)], query_embedding=e0)
    # the BM25 facade (its query is taken as it is: no city)
    bm = r.bm25.search('"alpha beta" -"alpha beta gamma"', top_k=50, phrases=True)
    assert bm and bm == r.bm25.search("alpha beta", top_k=50, within=DocSet.from_mask(ix, ab & ~abc))
    assert bm == r.bm25.search("alpha beta", top_k=50, must_phrases=["alpha beta"], must_not_phrases=[["alpha", "beta", "gamma"]])
    assert r.bm25.search('"alpha unknownword"', phrases=True) == []


def test_http_search_with_phrases(corp, eng):
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from msretr.server import create_app
    ix, off, tok, terms, qv = corp
    r = Retriever(indexer=eng)
    client = TestClient(create_app(r))
    body = {"query": '"alpha beta" -"beta alpha"', "top_k": 1000, "query_id": "q1", "query_embedding": qv[0].tolist()}
    plain = client.post("/api/search", json=body)
    phr = client.post("/api/search", json=dict(body, phrases=True))
    assert plain.status_code == 200 and phr.status_code == 200
    want = r.search(body["query"], top_k=1000, query_embedding=qv[0], query_id="q1", phrases=True)
    assert phr.json()["documents"] == want and want
    assert plain.json()["documents"] == r.search(body["query"], top_k=1000, query_embedding=qv[0], query_id="q1")
    assert plain.json()["documents"] != want
    lists = client.post("/api/search", json=dict(body, query="alpha beta", must_phrases=["alpha beta"],
                                                 must_not_phrases=["beta alpha"], mode="hybrid"))
    assert lists.status_code == 200
    assert lists.json()["documents"] == r.search("alpha beta", top_k=1000, query_embedding=qv[0], query_id="q1",
                                                 must_phrases=["alpha beta"], must_not_phrases=["beta alpha"], mode="hybrid")


def test_phrases_follow_add_remove_and_update_index():
    c = corpus(1025)
    r = Retriever(indexer=DeviceEngine(c.ix, max_queries=4, max_k=64, rerank_max_docs=0))
    try:
        ids = _np(c.ix.doc_ids)
        find = lambda p: set(r.engine.phrase_sets([[p]]).docset(0).indices().tolist())
        late = c.doc["late"]                                 # holds A B C
        assert late in find([A, B, C_]) and find([X, Y]) == set()
        new_ids = np.array([int(ids[-1]) + 5, int(ids[40]) + 1])              # appended and interleaved
        off = np.array([0, 4, 7], np.int64)
        tok = np.array([3, X, Y, 4, Y, X, Y], np.int32)
        ix2 = remove_documents(bm25_add_token_ids(c.ix, new_ids, off, tok, N_TERMS, device="cuda"), [int(ids[late])],
                               device="cuda")
        assert ix2.tok_off is not None and ix2.n_docs == 1026
        old = r.engine.phrase_sets([[[A, B]]])
        r.update_index(ix2)
        assert r.engine.has_tokens
        pos = {int(d): i for i, d in enumerate(_np(ix2.doc_ids))}
        assert find([X, Y]) == {pos[int(new_ids[0])], pos[int(new_ids[1])]}
        assert find([Y, X, Y]) == {pos[int(new_ids[1])]}
        want_abc = {pos[int(ids[d])] for d in np.nonzero(expected(1025)[1][[r_.claim for r_ in expected(1025)[0]].index(
            "A B C over the corpus")])[0] if d != late}
        assert find([A, B, C_]) == want_abc and int(ids[late]) not in pos
        with pytest.raises(ValueError, match="built for another index"):
            r.engine.bm25_topk([[A]], k=10, within=old)
        hits = r.bm25.search_terms([X], top_k=10, within=r.engine.phrase_sets([[[X, Y]]]))
        assert sorted(d for d, _ in hits) == sorted(int(v) for v in new_ids)
        # an update to an index without a forward index leaves no token binding behind
        bare = CorpusIndex(**{k: getattr(ix2, k) for k in ("doc_ids", "doc_len", "term_off", "post_doc", "post_tf", "idf", "avgdl",
                                                            "total_docs")})
        bare.n_docs_global = bare.n_docs
        r.update_index(bare)
        eng = r.engine
        assert not eng.has_tokens
        W = (bare.n_docs + 31) // 32
        p_off, p_terms, out = _i32([0, 2], eng.device), _i32([X, Y], eng.device), _filled(1, W, eng.device)
        assert eng.lib.msr_phrase_sets(eng.handle, 1, _P(p_off), _P(p_terms), _P(None), 0, 0, _P(None), _P(out), W, eng._stream()) == -2
        torch.cuda.synchronize(eng.device)
        assert (_host(out) == FILL).all()
        with pytest.raises(MsrError, match="attach_tokens"):
            eng.phrase_sets([[[X, Y]]])
        assert r.bm25.search_terms([Y], top_k=10)            # (a search without phrases goes on working)
    finally:
        r.engine.close()


def test_an_index_without_a_forward_index_refuses_phrases_and_searches_as_before(corp, eng):
    ix, off, tok, terms, qv = corp
    fields = {k: getattr(ix, k) for k in ("doc_ids", "doc_len", "term_off", "post_doc", "post_tf", "idf", "avgdl", "total_docs",
                                          "k1", "b", "vocab", "doc_off", "chunk_ids", "emb", "urls", "titles", "texts")}
    plain = CorpusIndex(**fields)
    plain.n_docs_global = plain.n_docs
    assert plain.tok_off is None
    r0, r1 = Retriever(indexer=DeviceEngine(plain, max_queries=16, max_k=1000, rerank_max_docs=1000)), Retriever(indexer=eng)
    try:
        assert not r0.engine.has_tokens
        for kw in (dict(phrases=True), dict(must_phrases=["alpha beta"])):
            with pytest.raises(MsrError, match="attach_tokens"):
                r0.search('"alpha beta"', query_embedding=qv[0], **kw)
        with pytest.raises(MsrError, match="attach_tokens"):
            r0.bm25.search('"alpha beta"', phrases=True)
        for mode in ("lexical", "hybrid"):
            a = r0.search('"alpha beta"', query_embedding=qv[0], mode=mode)
            assert a and a == r1.search('"alpha beta"', query_embedding=qv[0], mode=mode)
            assert a == r0.search('"alpha beta"', query_embedding=qv[0], mode=mode, phrases=False, must_phrases=None)
        _same(r0.final_lists(terms, qv, 1000), r1.final_lists(terms, qv, 1000))
    finally:
        r0.engine.close()
