"""Facet counts on the GPU (msr_bind_facet, msr_facet_counts, DeviceEngine.facet_counts, facets=True of the facades; DESIGN
K17): the kernels against the numpy reference of facet_ref.py on every hand-made corpus and value layout, element for element;
determinism; rows alone and in a batch; the bind's and the call's refusals; and the consumers -- Retriever.search_batch and
/api/search against the reference computed from facets.counting_terms and a host mask."""
import ctypes as C

import numpy as np
import pytest
import torch

from facet_ref import BIG, S, SIZES, base_mask, corpus, facet_counts_ref, facet_rows, top_ref, value_layouts
from msretr import _abi, facets
from msretr.chunk_index import ChunkTable, attach_chunks
from msretr.docset import DocSet, pack_bits
from msretr.engine import DeviceEngine
from msretr.index import CorpusIndex, _np
from msretr.index_build import attach_tokens, bm25_add_token_ids
from msretr.retriever import Retriever
from msretr.synthetic import synthetic_corpus
from phrase_ref import phrase_mask_fast
from term_set_ref import term_set_mask

pytestmark = pytest.mark.gpu
FILL = -1515870811                                           # 0xA5A5A5A5 as int32
PAD = 3                                                      # elements of a count row behind n_values that must keep the fill
INVALID, NOT_BOUND = -1, -2


def _P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _i32(a, dev):
    a = np.asarray(a, np.int32).reshape(-1)
    return torch.from_numpy(a if len(a) else np.zeros(1, np.int32)).to(dev)


def _filled(shape, dev):
    return torch.full(shape, FILL, dtype=torch.int32, device=dev)


def _base_rows(c, dev, extra=2):
    W = (c.n_docs + 31) // 32
    b = np.full((len(c.bases), W + extra), 0xFFFFFFFF, np.uint32)
    for i, (_, m) in enumerate(c.bases):
        b[i, :W] = pack_bits(m)
    return torch.from_numpy(b.view(np.int32)).to(dev), W + extra


def _pack(rows, dev):
    off, terms = [0], []
    for any_terms, _, _ in rows:
        terms += list(any_terms)
        off.append(len(terms))
    return _i32(off, dev), _i32(terms, dev), _i32([b for _, b, _ in rows], dev)


def _run(eng, c, rows, n_values, limit=10, counts=True, with_bases=True):
    """One msr_facet_counts call into pre-filled buffers with one row more than the call writes -> host arrays
    (hits [R + 1], n_values_hit [R + 1], top_value [R + 1, limit], top_count [R + 1, limit], counts [R + 1, n_values + PAD])."""
    dev, R = eng.device, len(rows)
    off, terms, rb = _pack(rows, dev)
    hits, n_hit = _filled((R + 1,), dev), _filled((R + 1,), dev)
    tv, tc = _filled((R + 1, max(limit, 1)), dev), _filled((R + 1, max(limit, 1)), dev)
    cnt = _filled((R + 1, n_values + PAD), dev) if counts else None
    need = eng.lib.msr_facet_scratch_bytes(eng.handle, R)
    assert need >= 0
    scratch = torch.empty((need // 8 + 2,), dtype=torch.int64, device=dev)
    bb, bs = _base_rows(c, dev) if with_bases else (None, 0)
    rc = eng.lib.msr_facet_counts(eng.handle, R, _P(off), _P(terms), _P(bb), len(c.bases) if with_bases else 0, bs,
                                  _P(rb) if with_bases else _P(None), limit, _P(hits), _P(n_hit), _P(tv) if limit else _P(None),
                                  _P(tc) if limit else _P(None), _P(cnt), n_values + PAD, _P(scratch), need, eng._stream())
    assert rc == 0, eng.lib.msr_last_error(eng.handle)
    torch.cuda.synchronize(dev)
    host = lambda t: None if t is None else t.cpu().numpy()
    return host(hits), host(n_hit), host(tv)[:, :limit], host(tc)[:, :limit], host(cnt)


def _reference(c, rows, value, n_values):
    """Computed once per (corpus, layout): [(hits, counts)] per row."""
    return [facet_counts_ref(c.z, value, n_values, a, base_mask(c, b)) for a, b, _ in rows]


def _check(rows, ref, got, n_values, limit, what):
    hits, n_hit, tv, tc, cnt = got
    R = len(rows)
    assert hits[R] == FILL and n_hit[R] == FILL, what        # the row behind the call's rows keeps the fill
    if limit:
        assert (tv[R] == FILL).all() and (tc[R] == FILL).all(), what
    if cnt is not None:
        assert (cnt[R] == FILL).all() and (cnt[:, n_values:] == FILL).all(), what
    for i, (_, _, claim) in enumerate(rows):
        w_hits, w_counts = ref[i]
        w_tv, w_tc, w_n = top_ref(w_counts, limit)
        assert hits[i] == w_hits and n_hit[i] == w_n, (what, claim, int(hits[i]), w_hits, int(n_hit[i]), w_n)
        assert (tv[i] == w_tv).all() and (tc[i] == w_tc).all(), (what, claim, tv[i].tolist(), w_tv.tolist())
        if cnt is not None:
            assert (cnt[i, :n_values] == w_counts).all(), (what, claim)
        assert w_counts.sum() <= w_hits


class Bound:
    """An engine over corpus(N), and the value layouts bound to it one after the other."""

    def __init__(self, N):
        self.c = corpus(N)
        self.eng = DeviceEngine(self.c.ix, max_queries=4, max_k=16, rerank_max_docs=0)
        self.layouts = value_layouts(N)
        self.rows = facet_rows(self.c)

    def bind(self, i):
        name, value, n_values = self.layouts[i]
        self.eng.bind_facet(value, n_values)
        return name, value, n_values


@pytest.fixture(scope="module")
def bound():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    made = {}

    def get(N):
        if N not in made:
            made[N] = Bound(N)
        return made[N]
    yield get
    for b in made.values():
        b.eng.close()


@pytest.mark.parametrize("N", SIZES)
def test_kernels_against_reference_every_layout(bound, N):
    b = bound(N)
    c, eng, rows = b.c, b.eng, b.rows
    for i in range(len(b.layouts)):
        name, value, n_values = b.bind(i)
        ref = _reference(c, rows, value, n_values)
        first = _run(eng, c, rows, n_values, limit=10)
        _check(rows, ref, first, n_values, 10, (N, name))
        again = _run(eng, c, rows, n_values, limit=10)       # a second call into second buffers: the same bytes
        assert all(x.tobytes() == y.tobytes() for x, y in zip(first, again)), (N, name)
        for limit in (0, 1, 64):                             # without out_counts: the same hits and top lists
            _check(rows, ref, _run(eng, c, rows, n_values, limit=limit, counts=False), n_values, limit, (N, name, limit))
        for j in (0, 7, len(rows) - 2):                      # a row alone equals the row inside the batch
            alone = _run(eng, c, rows[j:j + 1], n_values, limit=10)
            assert all((x[0] == y[j]).all() for x, y in zip(alone, first)), (N, name, rows[j][2])
    if N == 33:                                              # d % 3 at N = 33 ties; the tie resolves by value ascending
        name, value, n_values = b.bind(3)
        got = _run(eng, c, [([], -1, "all")], n_values, limit=3)
        counts = np.bincount(value[value >= 0], minlength=3)
        assert len(set(counts.tolist())) < 3 and got[2][0].tolist() == top_ref(counts, 3)[0].tolist()
    if N >= S:                                               # one value for all: a slot of the 16-bit partial counts exactly S
        name, value, n_values = b.bind(0)
        got = _run(eng, c, [([], -1, "all")], n_values, limit=1)
        assert got[0][0] == N and got[3][0, 0] == N and got[4][0, 0] == N


def test_batch_of_300_mixed_rows_and_no_bases(bound):
    b = bound(BIG)
    c, eng = b.c, b.eng
    name, value, n_values = b.bind(4)                        # the skewed layout
    rng = np.random.default_rng(9)
    rows = [b.rows[int(i)] for i in rng.integers(0, len(b.rows), 300)]
    ref = _reference(c, rows, value, n_values)
    got = _run(eng, c, rows, n_values, limit=10)
    _check(rows, ref, got, n_values, 10, "300 rows")
    for j in (3, 150, 299):
        alone = _run(eng, c, rows[j:j + 1], n_values, limit=10)
        assert all((x[0] == y[j]).all() for x, y in zip(alone, got)), rows[j][2]
    # n_base == 0: base_bits / row_base are NULL and not read, every row counts inside the whole corpus
    free = [(a, bb, claim) for a, bb, claim in b.rows[:40]]
    ref = [facet_counts_ref(c.z, value, n_values, a, None) for a, _, _ in free]
    _check(free, ref, _run(eng, c, free, n_values, limit=10, with_bases=False), n_values, 10, "no bases")


def _tables(value, n_values, dev):
    local, span_off, span_values, value_off, value_pos = facets.build_table(value, n_values)
    return [local.view(np.int16), span_off, span_values, value_off, value_pos]


def _bind_raw(eng, arrays, n_docs, n_values):
    dev = [torch.from_numpy(np.ascontiguousarray(a)).to(eng.device) for a in arrays]
    rc = eng.lib.msr_bind_facet(eng.handle, *[_P(t) for t in dev], n_docs, n_values, eng._stream())
    return rc, dev


def test_bind_refuses_malformed_tables_and_keeps_the_previous_binding(bound):
    b = bound(1025)
    c, eng = b.c, b.eng
    name, value, n_values = b.bind(4)
    rows = b.rows[:12]
    ref = _reference(c, rows, value, n_values)
    good = _tables(value, n_values, eng.device)

    def broken(i, fn):
        arrays = [a.copy() for a in good]
        fn(arrays[i])
        return arrays

    def bad_local(a):
        a[5] = good[1][1]                                    # a local id at the span's entry count

    def bad_span_values(a):
        a[3], a[4] = a[4], a[3]                              # not ascending

    def bad_value_pos(a):
        v = int(np.nonzero(np.diff(good[3]) > 0)[0][0])      # the first value with a slot ...
        a[good[3][v]] = int(np.nonzero(good[2] != v)[0][0])  # ... names a slot that holds another value

    def bad_value_off(a):
        a[-1] += 1
    cases = [broken(0, bad_local), broken(2, bad_span_values), broken(4, bad_value_pos), broken(3, bad_value_off)]
    for arrays in cases:
        rc, _ = _bind_raw(eng, arrays, c.n_docs, n_values)
        assert rc == INVALID and b"msr_bind_facet" in eng.lib.msr_last_error(eng.handle)
        _check(rows, ref, _run(eng, c, rows, n_values), n_values, 10, "after a refused bind")    # the previous binding answers
    rc, _ = _bind_raw(eng, good, c.n_docs + 1, n_values)     # a wrong n_docs
    assert rc == INVALID
    _check(rows, ref, _run(eng, c, rows, n_values), n_values, 10, "after a refused bind")
    rc, keep = _bind_raw(eng, good, c.n_docs, n_values)      # the table itself is sound
    assert rc == 0
    _check(rows, ref, _run(eng, c, rows, n_values), n_values, 10, "raw bind")
    b.bind(4)                                                # (the engine's own tensors again, before `keep` goes away)


def test_not_bound_and_unbinding():
    c = corpus(1025)
    eng = DeviceEngine(c.ix, max_queries=4, max_k=16, rerank_max_docs=0)
    try:
        dev = eng.device
        rows = facet_rows(c)[:3]
        off, terms, rb = _pack(rows, dev)
        outs = [_filled((3,), dev), _filled((3,), dev), _filled((3, 4), dev), _filled((3, 4), dev)]
        scratch = torch.empty((1 << 16,), dtype=torch.int64, device=dev)

        def call():
            return eng.lib.msr_facet_counts(eng.handle, 3, _P(off), _P(terms), _P(None), 0, 0, _P(None), 4, *[_P(o) for o in outs],
                                            _P(None), 0, _P(scratch), scratch.numel() * 8, eng._stream())
        untouched = lambda: all((o.cpu().numpy() == FILL).all() for o in outs)
        assert not eng.has_facet and call() == NOT_BOUND and untouched()                    # before any bind
        assert eng.lib.msr_facet_scratch_bytes(eng.handle, 3) == NOT_BOUND
        with pytest.raises(_abi.MsrError):
            eng.facet_counts([[0]])
        name, value, n_values = value_layouts(1025)[3]
        eng.bind_facet(value, n_values)
        assert eng.has_facet and call() == 0 and not untouched()
        for o in outs:
            o.fill_(FILL)
        eng.bind_facet(None, 0)                                                             # unbinding by NULL
        assert not eng.has_facet and call() == NOT_BOUND and untouched()
        eng.bind_facet(value, n_values)
        assert call() == 0
        torch.cuda.synchronize(dev)
        for o in outs:
            o.fill_(FILL)
        assert eng.lib.msr_unbind(eng.handle) == 0                                          # msr_unbind drops the binding
        assert call() == NOT_BOUND and untouched()
        null = C.c_void_p(0)
        assert eng.lib.msr_bind_facet(eng.handle, null, null, null, null, null, 0, 0, eng._stream()) == NOT_BOUND   # no postings
        eng.rebind(c.ix)                                                                    # a rebind comes without a facet
        assert not eng.has_facet and call() == NOT_BOUND
    finally:
        eng.close()


def test_call_refusals_leave_the_outputs_untouched(bound):
    b = bound(1025)
    c, eng = b.c, b.eng
    name, value, n_values = b.bind(4)
    dev, lib, h, st = eng.device, eng.lib, eng.handle, eng._stream()
    rows = b.rows[:4]
    off, terms, rb = _pack(rows, dev)
    bb, bs = _base_rows(c, dev)
    W = (c.n_docs + 31) // 32
    outs = dict(hits=_filled((4,), dev), nh=_filled((4,), dev), tv=_filled((4, 10), dev), tc=_filled((4, 10), dev),
                cnt=_filled((4, n_values), dev))
    need = lib.msr_facet_scratch_bytes(h, 4)
    assert need == 4 * ((2 * len(facets.build_table(value, n_values)[2]) + 15) // 16 * 16 + 4 * ((c.n_docs + S - 1) // S))
    assert lib.msr_facet_scratch_bytes(h, 0) == 0 and lib.msr_facet_scratch_bytes(h, -1) == INVALID
    scratch = torch.empty((need // 8 + 2,), dtype=torch.int64, device=dev)
    good = dict(n=4, off=off, bb=bb, nb=len(c.bases), bs=bs, rb=rb, limit=10, cs=n_values, sb=need, scratch=scratch, **outs)
    bad = [dict(n=-1), dict(limit=-1), dict(limit=_abi.MSR_FACET_MAX_LIMIT + 1), dict(off=None), dict(hits=None), dict(nh=None),
           dict(tv=None), dict(tc=None), dict(cs=n_values - 1), dict(sb=need - 1), dict(scratch=None), dict(nb=-1), dict(bb=None),
           dict(rb=None), dict(bs=W - 1)]

    def call(a):
        return lib.msr_facet_counts(h, a["n"], _P(a["off"]), _P(terms), _P(a["bb"]), a["nb"], a["bs"], _P(a["rb"]), a["limit"],
                                    _P(a["hits"]), _P(a["nh"]), _P(a["tv"]), _P(a["tc"]), _P(a["cnt"]), a["cs"], _P(a["scratch"]),
                                    a["sb"], st)
    for change in bad:
        assert call(dict(good, **change)) == INVALID, change
        assert b"msr_facet_counts" in lib.msr_last_error(h)
        torch.cuda.synchronize(dev)
        assert all((o.cpu().numpy() == FILL).all() for o in outs.values()), change
    # n_rows == 0 succeeds and launches nothing, whatever the pointers
    assert lib.msr_facet_counts(h, 0, _P(None), _P(None), _P(None), 0, 0, _P(None), 10, _P(None), _P(None), _P(None), _P(None),
                                _P(None), 0, _P(None), 0, st) == 0
    assert call(dict(good, n=0)) == 0
    torch.cuda.synchronize(dev)
    assert all((o.cpu().numpy() == FILL).all() for o in outs.values())
    assert call(good) == 0                                   # and the call itself is sound
    torch.cuda.synchronize(dev)
    assert (outs["hits"].cpu().numpy() != FILL).all()
    with pytest.raises(ValueError):
        eng.facet_counts([[0]], limit=65)


def test_engine_facet_counts_in_slices(bound):
    b = bound(BIG)
    c, eng = b.c, b.eng
    name, value, n_values = b.bind(4)
    assert eng.max_queries == 4
    t = c.term
    lists = [[t["even"]], [t["rnd1"], t["rnd30"]], [], [t["all"]], [-1], [t["skipper"], t["n2048"]], [t["one_0"]], [t["empty"]],
             [t["rnd30"], t["rnd30"]]]
    odd = DocSet.from_mask(c.ix, c.bases[0][1])
    within = [None, odd, odd, None, None, odd, None, None, odd]
    got = eng.facet_counts(lists, within=within, limit=5, counts=True)
    assert [g.shape for g in got] == [(9,), (9,), (9, 5), (9, 5), (9, n_values)]
    for q in range(9):
        one = eng.facet_counts(lists[q:q + 1], within=within[q], limit=5, counts=True)
        assert all((o[0] == g[q]).all() for o, g in zip(one, got)), q
        hits, counts = facet_counts_ref(c.z, value, n_values, lists[q], None if within[q] is None else within[q].mask)
        assert got[0][q] == hits and (got[4][q] == counts).all() and (got[2][q] == top_ref(counts, 5)[0]).all()
    ds = eng.term_sets([[t["even"]]] * 9, within=within)     # a DeviceSets as the base rows
    dg = eng.facet_counts(lists, within=ds, limit=5)
    for q in range(9):
        m = term_set_mask(c.z, [t["even"]], [], None if within[q] is None else within[q].mask)
        assert dg[0][q] == facet_counts_ref(c.z, value, n_values, lists[q], m)[0]
    assert len(eng.facet_counts([], limit=5)[0]) == 0


# ------------------------------------------------------------------------------------------------ consumers
N_DOCS = 2000
HOSTS = ["uni-tuebingen.de", "www.tuebingen.de", "tuebingen.de", "example.org"] + [f"s{i}.example.net" for i in range(40)]


def _word(t):
    s, t = "", int(t)
    while True:
        s = chr(ord("a") + t % 26) + s
        t //= 26
        if t == 0:
            return "w" + s


def _streams(ix):
    """A forward index that agrees with the postings: every document's terms ascending, each tf times."""
    off, doc, tf = _np(ix.term_off).astype(np.int64), _np(ix.post_doc).astype(np.int64), _np(ix.post_tf).astype(np.int64)
    term = np.repeat(np.arange(len(off) - 1), np.diff(off))
    order = np.lexsort((term, doc))
    tok = np.repeat(term[order], tf[order]).astype(np.int32)
    lens = np.bincount(doc, weights=tf, minlength=ix.n_docs).astype(np.int64)
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), tok


@pytest.fixture(scope="module")
def site():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    ix = synthetic_corpus(N_DOCS, n_chunks=6000, n_terms=3000, seed=31)
    rng = np.random.default_rng(32)
    w = 1.0 / (1.0 + np.arange(len(HOSTS))) ** 1.2
    host = rng.choice(len(HOSTS), N_DOCS, p=w / w.sum())
    ids = _np(ix.doc_ids)
    ix.urls = [None if d % 97 == 5 else f"https://{HOSTS[host[d]]}/doc{int(ids[d])}" for d in range(N_DOCS)]
    ix.titles = [f"title {d}" for d in range(N_DOCS)]
    ix.texts = [f"text of document {d} " * 3 for d in range(N_DOCS)]
    ix._url_group = None
    z = {"term_off": _np(ix.term_off).astype(np.int64), "post_doc": _np(ix.post_doc), "n_docs": N_DOCS}
    df = np.diff(z["term_off"])
    by_df = np.argsort(-df, kind="stable")
    mid = [int(t) for t in by_df[100:140]]
    assert 0 not in mid and df[mid[0]] < N_DOCS // 2
    names = {t: _word(t) for t in range(ix.n_terms)}         # one name per term
    names.update({0: "tübingen", mid[20]: "mensa", mid[21]: "bibliothek", mid[22]: "bibliothekar"})
    ix.vocab = {name: t for t, name in names.items()}
    attach_tokens(ix, *_streams(ix))
    g = torch.Generator().manual_seed(33)
    qv = torch.randn((8, 768), generator=g).numpy()
    r = Retriever(indexer=ix, max_queries=8, max_k=1000)
    yield ix, z, mid, qv, r
    r.engine.close()


def _want(ix, z, ids, mask, by, limit):
    """(hits, facets, facet_values) of the reference: the counting terms of `ids` inside `mask`."""
    value, names = facets.facet_values(ix, by)
    counting = facets.counting_terms(ix, ids)
    if not counting:
        return 0, [], 0
    hits, counts = facet_counts_ref(z, value, len(names), counting, mask)
    tv, tc, n_hit = top_ref(counts, limit)
    assert counts.sum() <= hits
    return hits, facets.top_list(names, tv, tc), n_hit


def _same_facets(res, want):
    assert (res.hits, res.facets, res.facet_values) == want, (res.hits, res.facets[:3], want[0], want[1][:3])


@pytest.mark.parametrize("by", ["host", "domain"])
def test_search_batch_facets_against_the_reference(site, by):
    ix, z, mid, qv, r = site
    V = ix.vocab
    A, B, M = mid[1], mid[9], V["mensa"]
    wa, wb = _word(A), _word(B)
    w1, w2 = _word(30), _word(31)                            # frequent words with adjacent ids stand next to each other where both are
    off, tok = _np(ix.tok_off), _np(ix.tok_ids)
    uni = DocSet.from_sites(ix, ["uni-tuebingen.de"])
    # plain, in one batch of 8: the rows equal the call without facets
    qs = ["mensa", f"mensa {wa}", f"{wa} {wb}", "tübingen", "zzzz qqqq", f"bibliothek {wb}", f"{wb}", f"mensa bibliothek {wa}"]
    id_lists = [[M, 0], [M, A, 0], [A, B, 0], [0, 0], [-1, -1, 0], [V["bibliothek"], B, 0], [B, 0], [M, V["bibliothek"], A, 0]]
    got = r.search_batch(qs, query_embeddings=qv, facets=True, facet_by=by, facet_limit=6)
    assert got == r.search_batch(qs, query_embeddings=qv)
    for q in range(8):
        _same_facets(got[q], _want(ix, z, id_lists[q], None, by, 6))
        assert sum(f["count"] for f in got[q].facets) <= got[q].hits
    assert got[0].hits > 100                                 # counted over all matches, not over the ~100 rows returned
    if by == "host":
        assert len(got[0].facets) == 6 and got[0].facet_values > 6
    else:                                                    # three names in all: example.org and *.example.net share "example"
        assert len(got[0].facets) == got[0].facet_values == 3
    assert got[3].hits > N_DOCS // 2                          # only the city: no positive idf, so the city counts
    unknown = r.search("zzzz qqqq", query_embedding=qv[4], terms=["zzzz", "qqqq"], facets=True, facet_by=by)
    assert unknown == [] and unknown.hits == 0 and unknown.facets == [] and unknown.facet_values == 0
    # within a site set
    res = r.search("mensa", query_embedding=qv[0], within=uni, facets=True, facet_by=by)
    _same_facets(res, _want(ix, z, [M, 0], uni.mask, by, 10))
    if by == "host":
        assert [f["value"] for f in res.facets] == ["uni-tuebingen.de"] and res.hits == res.facets[0]["count"]
        top = got[0].facets[0]                               # a facet value handed back as a site restricts to its pages
        back = r.search("mensa", query_embedding=qv[0], within=DocSet.from_sites(ix, [top["value"]]), facets=True)
        assert back.hits >= top["count"] and {"value": top["value"], "count": top["count"]} in back.facets
    # operators: a must and a must_not term
    res = r.search(f"mensa +{wa} -{wb}", query_embedding=qv[1], operators=True, facets=True, facet_by=by)
    assert res == r.search(f"mensa +{wa} -{wb}", query_embedding=qv[1], operators=True)
    _same_facets(res, _want(ix, z, [M, A, 0], term_set_mask(z, [A], [B]), by, 10))
    # phrases
    res = r.search(f'mensa "{w1} {w2}"', query_embedding=qv[2], phrases=True, facets=True, facet_by=by)
    ph = phrase_mask_fast(off, tok, [30, 31], None, ix.n_terms)
    assert 0 < ph.sum() < N_DOCS
    _same_facets(res, _want(ix, z, [M, 30, 31, 0], ph, by, 10))
    # fuzzy: the corrected term is the one counted
    res = r.search("mensaa", query_embedding=qv[3], fuzzy=True, facets=True, facet_by=by)
    assert res.corrections == {"mensaa": "mensa"}
    _same_facets(res, _want(ix, z, [M, 0], None, by, 10))
    # wildcards: the expansions are counted
    res = r.search("bibliothek*", query_embedding=qv[5], wildcards=True, facets=True, facet_by=by)
    used = [V[t] for t in res.expansions["bibliothek*"]["terms"]]
    assert sorted(used) == sorted([V["bibliothek"], V["bibliothekar"]])
    _same_facets(res, _want(ix, z, [0] + used, None, by, 10))
    # hybrid mode counts the lexical matches only
    res = r.search("mensa", query_embedding=qv[0], mode="hybrid", facets=True, facet_by=by)
    _same_facets(res, _want(ix, z, [M, 0], None, by, 10))
    for bad in (dict(facet_limit=0), dict(facet_limit=65), dict(facet_by="tld")):
        with pytest.raises(ValueError):
            r.search("mensa", query_embedding=qv[0], facets=True, **bad)


def test_facets_need_urls():
    ix = synthetic_corpus(300, n_chunks=600, n_terms=500, seed=5)
    r = Retriever(indexer=ix, max_queries=4, max_k=100, rerank_max_docs=100)
    try:
        with pytest.raises(ValueError, match="URLs"):
            r.search_batch(["q"], top_k=100, query_embeddings=np.zeros((1, 768), np.float32), term_lists=[["x"]], facets=True)
    finally:
        r.engine.close()


def test_http_search_with_facets(site):
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from msretr.server import create_app
    ix, z, mid, qv, r = site
    client = TestClient(create_app(r))
    body = {"query": "mensa", "top_k": 1000, "query_id": "q1", "query_embedding": qv[0].tolist()}
    plain = client.post("/api/search", json=body)
    got = client.post("/api/search", json=dict(body, facets=True, facet_limit=4, sites=["tuebingen.de"]))
    assert plain.status_code == 200 and got.status_code == 200 and "hits" not in plain.json()
    want = r.search("mensa", top_k=1000, query_embedding=qv[0], query_id="q1", facets=True, facet_limit=4,
                    within=DocSet.from_sites(ix, ["tuebingen.de"]))
    out = got.json()
    assert out["documents"] == list(want) and want
    assert (out["hits"], out["facets"], out["facet_values"]) == (want.hits, want.facets, want.facet_values)
    assert {f["value"] for f in out["facets"]} <= {"uni-tuebingen.de", "www.tuebingen.de", "tuebingen.de"} and out["hits"] > 0
    assert client.post("/api/search", json=dict(body, facets=True, facet_limit=0)).status_code == 400
    assert client.post("/api/search", json=dict(body, facets=True, facet_by="tld")).status_code == 400


def test_counts_follow_update_index(site):
    ix, z, mid, qv, _ = site
    r = Retriever(indexer=ix, max_queries=8, max_k=1000)
    try:
        M = ix.vocab["mensa"]
        before = r.search("mensa", query_embedding=qv[0], facets=True)
        _same_facets(before, _want(ix, z, [M, 0], None, "host", 10))
        # 40 new pages of a new site, every one holding the word
        new_ids = np.arange(40, dtype=np.int64) + int(_np(ix.doc_ids).max()) + 10
        off = np.arange(41, dtype=np.int64) * 3
        tok = np.tile(np.asarray([M, 5, 7], np.int32), 40)
        meta = {int(d): (f"https://new.example.com/p{int(d)}", f"T{int(d)}", f"text {int(d)}") for d in new_ids}
        grown = bm25_add_token_ids(ix, new_ids, off, tok, ix.n_terms, vocab=ix.vocab, docs_meta=meta)
        e = torch.randn((40, 768), generator=torch.Generator().manual_seed(1))
        first = int(_np(ix.chunk_ids).max()) + 1
        grown = attach_chunks(grown, ChunkTable(chunk_ids=np.arange(first, first + 40, dtype=np.int64), doc_ids=new_ids,
                                                seqs=[[1]] * 40, emb=e / e.norm(dim=1, keepdim=True)))
        r.update_index(grown)
        after = r.search("mensa", query_embedding=qv[0], facets=True, facet_limit=64)
        z2 = {"term_off": _np(grown.term_off).astype(np.int64), "post_doc": _np(grown.post_doc), "n_docs": grown.n_docs}
        _same_facets(after, _want(grown, z2, [M, 0], None, "host", 64))
        assert after.hits == before.hits + 40 and {"value": "new.example.com", "count": 40} in after.facets
    finally:
        r.engine.close()
