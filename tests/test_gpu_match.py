"""Match modes on the GPU (msr_match_sets, match.match_sets, the match= option of the facades; DESIGN K19): the kernel against
the numpy oracle of match_ref.py, byte for byte, on an index of three spans (the last partial, N % 32 != 0) with heavy, light
and empty lists and unknown ids; the refusals; the cross-checks against msr_term_sets and msr_facet_counts, which have no
oracle in the loop; a caller's stream behind pending work; and the engine call and the facades against the same call inside a
host-built DocSet of the oracle's set."""
import ctypes as C

import numpy as np
import pytest
import torch

from match_ref import group_mask, match_mask, pack
from msretr import match as mt
from msretr._abi import MSR_MATCH_MAX_GROUPS, MSR_TERMSET_SPAN_DOCS
from msretr.docset import DeviceSets, DocSet
from msretr.engine import DeviceEngine, count_nonzero_words
from msretr.fuzzy import Results
from msretr.index import CorpusIndex, _np
from msretr.retriever import Retriever
from msretr.synthetic import synthetic_corpus, synthetic_queries
from term_set_ref import HEAVY_DF, term_set_mask

pytestmark = pytest.mark.gpu
FILL = 0xA5A5A5A5
PAD = 3                                                      # words of a row behind ceil(N / 32) that must keep the fill
N_DOCS = 20_013
W = (N_DOCS + 31) // 32
CARRY = (1, 2, 3, 4, 7, 8, 15, 16, 31, 32, 63)               # counts at which the ripple carry reaches a new plane, and one below
NAMED = ("mensa", "mensaria", "morgenstelle", "öffnungszeiten")


def _P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _i32(a, dev):
    return torch.from_numpy(np.asarray(a if len(a) else [0], np.int32)).to(dev)


def _word(t):
    s = ""
    t = int(t)
    while True:
        s = chr(ord("a") + t % 26) + s
        t //= 26
        if t == 0:
            return "w" + s


class Corp:
    pass


@pytest.fixture(scope="module")
def corp():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert N_DOCS % 32 and 2 * MSR_TERMSET_SPAN_DOCS < N_DOCS < 3 * MSR_TERMSET_SPAN_DOCS
    c = Corp()
    ix = c.ix = synthetic_corpus(N_DOCS, n_chunks=60_000, n_terms=150_000, seed=19)
    c.terms, qv = synthetic_queries(ix, 12, seed=12, lo_rank=5, hi_rank=3000)
    c.qv = qv.numpy()
    ids = _np(ix.doc_ids)
    hosts = ["uni-tuebingen.de", "tuebingen.de", "example.org"]
    ix.urls = [f"https://{hosts[d % 3]}/doc{int(ids[d])}" for d in range(N_DOCS)]
    ix.titles = [f"title {d}" for d in range(N_DOCS)]
    ix.texts = [f"text of document {d} " * 3 for d in range(N_DOCS)]
    ix._url_group = None
    c.z = {"term_off": _np(ix.term_off).astype(np.int64), "post_doc": _np(ix.post_doc), "n_docs": N_DOCS}
    df = c.df = np.diff(c.z["term_off"])
    by_df = np.argsort(-df, kind="stable")
    c.mid = [int(t) for t in by_df[100:180]]                 # about a quarter of the documents each: heavy lists, idf > 0
    c.light = [int(t) for t in by_df[600:700]]               # below the skip-table threshold
    c.rare = [int(t) for t in by_df[3000:3400]]
    c.empty = int(np.nonzero(df == 0)[0][0])
    assert df[c.mid[-1]] >= HEAVY_DF > df[c.light[0]] and df[c.rare[-1]] > 0 and df[0] >= HEAVY_DF and float(ix.idf[0]) < 0
    assert all(float(ix.idf[t]) > 0 for t in c.mid + c.light)
    names = {t: _word(t) for t in range(ix.n_terms)}
    names[0] = "tübingen"
    c.named = dict(zip(NAMED, c.mid[20:24]))
    for name, t in c.named.items():
        names[t] = name
    ix.vocab = {name: t for t, name in names.items()}
    c.V = int(ix.n_terms)
    rng = np.random.default_rng(5)
    c.bases = [np.arange(N_DOCS) % 2 == 1, np.arange(N_DOCS) >= (N_DOCS - 1) // 32 * 32, rng.random(N_DOCS) < 0.5]
    c.pos = {str(int(d)): i for i, d in enumerate(ids)}
    c.masks = {}
    return c


@pytest.fixture(scope="module")
def eng(corp):
    e = DeviceEngine(corp.ix, max_queries=16, max_k=1000, rerank_max_docs=1000)
    yield e
    e.close()


def _want(c, groups, need, base=-1, n_base=3):
    """The oracle's words of one row (group masks kept: many rows share their groups)."""
    bm = None if base == -1 or n_base == 0 else c.bases[base] if 0 <= base < n_base else np.zeros(N_DOCS, bool)
    if need <= 0 or len(groups) > MSR_MATCH_MAX_GROUPS or need > len(groups):
        return pack(match_mask(c.z, groups, need, bm))
    count = np.zeros(N_DOCS, np.int64)
    for g in groups:
        key = tuple(g)
        if key not in c.masks:
            c.masks[key] = group_mask(c.z, g)
        count += c.masks[key]
    return pack((count >= need) & (np.ones(N_DOCS, bool) if bm is None else bm))


def _pack_rows(rows, dev):
    g_off, t_off, terms = [0], [0], []
    for groups, _, _ in rows:
        for g in groups:
            terms += [int(t) for t in g]
            t_off.append(len(terms))
        g_off.append(len(t_off) - 1)
    return (_i32(g_off, dev), _i32(t_off, dev), _i32(terms, dev), _i32([n for _, n, _ in rows], dev),
            _i32([b for _, _, b in rows], dev))


def _base_rows(c, dev, extra=2):
    b = np.full((len(c.bases), W + extra), 0xFFFFFFFF, np.uint32)                 # (base_stride > ceil(N / 32), ones behind)
    for i, m in enumerate(c.bases):
        b[i, :W] = pack(m)
    return torch.from_numpy(b.view(np.int32)).to(dev), W + extra


def _run(eng, c, rows, with_bases=True):
    """One msr_match_sets call into a sentinel-filled buffer of stride W + PAD -> uint32 [R, W + PAD] (host)."""
    dev = eng.device
    out = torch.from_numpy(np.full((len(rows), W + PAD), FILL, np.uint32).view(np.int32)).to(dev)
    g_off, t_off, terms, need, rb = _pack_rows(rows, dev)
    bb, bs = _base_rows(c, dev) if with_bases else (None, 0)
    rc = eng.lib.msr_match_sets(eng.handle, len(rows), _P(g_off), _P(t_off), _P(terms), _P(need), _P(bb),
                                len(c.bases) if with_bases else 0, bs, _P(rb) if with_bases else _P(None), _P(out), W + PAD,
                                eng._stream())
    assert rc == 0, eng.lib.msr_last_error(eng.handle)
    torch.cuda.synchronize(dev)
    return out.cpu().numpy().view(np.uint32)


def _check(c, rows, got, with_bases=True):
    assert got.shape == (len(rows), W + PAD)
    assert (got[:, W:] == FILL).all(), "words behind ceil(N / 32) were touched"
    for i, (groups, need, base) in enumerate(rows):
        want = _want(c, groups, need, base, 3 if with_bases else 0)
        assert got[i, :W].tobytes() == want.tobytes(), (i, len(groups), need, base)
    assert (got[:, W - 1] >> np.uint32(N_DOCS % 32) == 0).all(), "bits at or above N"


def _rows(c):
    """The rows of the issue's list, each (groups, need, row_base)."""
    V, mid, light, rare = c.V, c.mid, c.light, c.rare
    pool = [mid[0], light[0], mid[1], light[1], mid[2], light[2], mid[3], 0] + mid[4:32] + light[3:31]      # 64 distinct terms
    assert len(set(pool)) == 64
    R = []
    for G in (1, 2, 3, 7, 8, 64):
        for need in sorted({1, (G + 1) // 2, G}):
            R.append(([[t] for t in pool[:G]], need, -1))
    # one document set in all 64 groups: its count is 64, the top plane
    R.append(([[t, light[40]] for t in pool], 64, -1))
    R.append(([[t, light[40]] for t in pool], 63, -1))
    # the carry edges: the documents of light[50 + k] alone reach exactly CARRY[k] of the 64 groups
    edge = [[light[50 + k] for k, cnt in enumerate(CARRY) if cnt > j] for j in range(64)]
    for cnt in CARRY:
        R.append((edge, cnt, -1))
        R.append((edge, cnt + 1, -1))
    # a group of 300 terms (two rounds of 256), an empty group, a group of unknown ids only
    big = rare[:300]
    for need in (1, 2, 3, 4):
        R.append(([big, [], [-1, V, V + 1000, -7], [mid[5]], [light[5], c.empty]], need, -1))
    R.append(([rare[:256]], 1, -1))
    R.append(([rare[:257], rare[100:400]], 2, -1))
    # one document in two terms of one group counts once; one term in two groups counts in both
    R.append(([[mid[6], mid[7]], [mid[8]]], 2, -1))
    R.append(([[mid[6], mid[6], mid[7]], [mid[8]]], 1, -1))
    R.append(([[mid[6]], [mid[6]], [mid[8]]], 2, -1))
    R.append(([[mid[6]], [mid[6]], [mid[8]]], 3, -1))
    # need <= 0, need = G + 1, 65 groups, a row with no groups
    R += [([[mid[9]], [mid[10]]], 0, -1), ([[mid[9]], [mid[10]]], -5, 0), ([[mid[9]], [mid[10]]], 3, -1)]
    R += [([[t] for t in pool] + [[mid[40]]], 1, -1), ([[t] for t in pool] + [[mid[40]]], 0, -1), ([], 1, -1), ([], 0, -1), ([], 0, 2)]
    # the empty list, the city's list (nearly every document), unknown words
    R += [([[c.empty]], 1, -1), ([[0]], 1, -1), ([[0], [c.empty], [mid[11]]], 2, -1), ([[-1]], 1, -1), ([[V], [mid[11]]], 1, -1),
          ([[V], [mid[11]]], 2, -1)]
    # bases: -1, every valid row, the row count itself, below -1
    for base in (0, 1, 2, 3, -2):
        R.append(([[mid[12]], [mid[13]], [light[6]]], 2, base))
        R.append(([[mid[12]], [mid[13]], [light[6]]], 3, base))
    R.append(([[0]], 1, 1))                                  # a base with bits only in the last word
    return R


def test_kernel_against_the_oracle_byte_for_byte(corp, eng):
    rows = _rows(corp)
    a = _run(eng, corp, rows)
    _check(corp, rows, a)
    assert _run(eng, corp, rows).tobytes() == a.tobytes()    # a second call, a second buffer: the same bytes
    nz = sum(int(r[:W].any()) for r in a)
    assert 30 <= nz <= len(rows) - 12, nz                    # the rows hold empty sets and non-empty ones
    # the carry rows say what they claim: at need = count the documents of that list alone are in, at count + 1 they are out
    first = next(i for i, r in enumerate(rows) if len(r[0]) == 64 and r[0][62] == [corp.light[50 + len(CARRY) - 1]])
    for k, cnt in enumerate(CARRY):
        docs = corp.z["post_doc"][corp.z["term_off"][corp.light[50 + k]]:corp.z["term_off"][corp.light[50 + k] + 1]]
        at, above = a[first + 2 * k], a[first + 2 * k + 1]
        bit = lambda row, d: int(row[d >> 5]) >> (d & 31) & 1
        assert all(bit(at, int(d)) for d in docs), cnt
        higher = set(np.concatenate([group_mask(corp.z, [corp.light[50 + j]]).nonzero()[0] for j in range(k + 1, len(CARRY))] or
                                    [np.zeros(0, np.int64)]).tolist())
        assert all(bit(above, int(d)) == (int(d) in higher) for d in docs), cnt
    # one row per call gives the same words as the row inside the batch
    for i in (0, 17, first + 3, len(rows) - 2):
        assert (_run(eng, corp, rows[i:i + 1])[0] == a[i]).all(), i


def test_dense_lists_behind_an_exit_check(corp, eng):
    """Rows whose LAST lists are the densest of the index (the city's: 85 % of the documents; term 1: nearly all), read behind
    groups that leave every span alive: thousands of ORs per span are in flight around each barrier of the group loop.  A
    barrier that does not wait for them loses bits, differently on every run (seen while this kernel was written)."""
    c = corp
    rows = [([[c.mid[i]], [0]], 2, -1) for i in range(40)] + [([[c.light[i]], [0], [1]], 3, -1) for i in range(20)] + \
           [([[c.mid[i]], [0], [1], [c.mid[i + 1]]], 3, 2) for i in range(20)]
    a = _run(eng, c, rows)
    _check(c, rows, a)
    assert all(r[:W].any() for r in a)
    for _ in range(3):
        assert _run(eng, c, rows).tobytes() == a.tobytes()


def test_without_bases_row_base_is_not_read(corp, eng):
    rows = [(g, n, b) for g, n, _ in _rows(corp)[:12] for b in (-1, 0, 7)]
    got = _run(eng, corp, rows, with_bases=False)
    _check(corp, rows, got, with_bases=False)


def test_refusals_leave_the_output_untouched(corp, eng):
    lib, h, st, dev = eng.lib, eng.handle, eng._stream(), eng.device
    rows = _rows(corp)[:4]
    g_off, t_off, terms, need, rb = _pack_rows(rows, dev)
    bb, bs = _base_rows(corp, dev)
    out = torch.from_numpy(np.full((4, W), FILL, np.uint32).view(np.int32)).to(dev)
    untouched = lambda: bool((out.cpu().numpy().view(np.uint32) == FILL).all())
    good = dict(n=4, g_off=g_off, t_off=t_off, need=need, bb=bb, nb=3, bs=bs, rb=rb, out=out, os=W)
    call = lambda a: lib.msr_match_sets(h, a["n"], _P(a["g_off"]), _P(a["t_off"]), _P(terms), _P(a["need"]), _P(a["bb"]), a["nb"],
                                        a["bs"], _P(a["rb"]), _P(a["out"]), a["os"], st)
    for change in (dict(n=-1), dict(out=None), dict(g_off=None), dict(t_off=None), dict(need=None), dict(os=W - 1), dict(bs=W - 1),
                   dict(nb=-1), dict(bb=None), dict(rb=None)):
        assert call(dict(good, **change)) == -1, change
        assert b"msr_match_sets" in lib.msr_last_error(h)
        torch.cuda.synchronize(dev)
        assert untouched(), change
    # n_rows == 0 succeeds (whatever the pointers) and launches nothing
    null = _P(None)
    assert lib.msr_match_sets(h, 0, null, null, null, null, null, 0, 0, null, null, W, st) == 0
    assert call(dict(good, n=0)) == 0
    torch.cuda.synchronize(dev)
    assert untouched()
    assert call(dict(good, bb=None, nb=0, bs=0, rb=None)) == 0           # base_stride is not looked at without bases
    torch.cuda.synchronize(dev)
    assert not untouched()
    bare = DeviceEngine(CorpusIndex(doc_ids=np.arange(5, dtype=np.int64)), max_queries=4, max_k=16, rerank_max_docs=0)
    try:                                                     # without postings: not bound
        assert bare.lib.msr_match_sets(bare.handle, 4, _P(g_off), _P(t_off), _P(terms), _P(need), null, 0, 0, null, _P(out), W,
                                       bare._stream()) == -2
    finally:
        bare.close()


# ------------------------------------------------------------------------------------------------ against the existing kernels
def test_singleton_groups_all_equal_term_sets(corp, eng):
    c, dev = corp, eng.device
    musts = [[c.mid[0]], [c.mid[1], c.light[0]], [c.light[1], c.mid[2], c.mid[3]], [c.mid[4], c.empty], [c.mid[5], -1],
             [0, c.mid[6], c.light[2], c.rare[0]], c.mid[10:18]]
    rows = [([[t] for t in m], len(m), b) for m in musts for b in (-1, 2)]
    got = _run(eng, c, rows)
    out = torch.from_numpy(np.full((len(rows), W + PAD), FILL, np.uint32).view(np.int32)).to(dev)
    m_off, m, x_off = [0], [], [0] * (len(rows) + 1)
    for groups, _, _ in rows:
        m += [g[0] for g in groups]
        m_off.append(len(m))
    bb, bs = _base_rows(c, dev)
    d_moff, d_m, d_xoff, d_rb = _i32(m_off, dev), _i32(m, dev), _i32(x_off, dev), _i32([b for _, _, b in rows], dev)
    rc = eng.lib.msr_term_sets(eng.handle, len(rows), _P(d_moff), _P(d_m), _P(d_xoff), _P(None), _P(bb), 3, bs, _P(d_rb), _P(out),
                               W + PAD, eng._stream())
    assert rc == 0, eng.lib.msr_last_error(eng.handle)
    torch.cuda.synchronize(dev)
    assert out.cpu().numpy().view(np.uint32).tobytes() == got.tobytes()
    assert sum(int(r[:W].any()) for r in got) >= 6


def test_need_one_is_the_or_that_facet_counts_counts(corp, eng):
    c = corp
    lists = [[c.mid[0], c.mid[1], c.light[0]], [c.light[1]], [c.rare[0], c.rare[1], c.empty, -1], [0, c.mid[2]], [c.empty]]
    rows = [([[t] for t in l], 1, b) for l in lists for b in (-1, 0)]
    got = _run(eng, c, rows)
    _check(c, rows, got)
    eng.bind_facet(np.arange(N_DOCS, dtype=np.int32) % 7, 7)
    try:
        odd = DocSet.from_mask(c.ix, c.bases[0])
        hits = eng.facet_counts([l for l in lists for _ in (0, 1)], within=[None, odd] * len(lists), limit=3)[0]
    finally:
        eng.bind_facet(None, 0)
    pop = [int(np.unpackbits(r[:W].view(np.uint8)).sum()) for r in got]
    assert hits.tolist() == pop and pop[0] > pop[1] > 0 and pop[-1] == 0
    dev_rows = torch.from_numpy(got[:, :W].copy().view(np.int32)).to(eng.device)
    for i in range(len(rows)):
        assert count_nonzero_words(dev_rows[i]) == int((got[i, :W] != 0).sum())


def test_a_callers_stream_behind_pending_work(corp, eng):
    c, dev = corp, eng.device
    rows = _rows(c)[:40]
    want = _run(eng, c, rows)                                # on the current (null) stream
    g_off, t_off, terms, need, rb = _pack_rows(rows, dev)
    bb, bs = _base_rows(c, dev)
    out = torch.from_numpy(np.full((len(rows), W + PAD), FILL, np.uint32).view(np.int32)).to(dev)
    ballast = torch.empty((64 << 20,), dtype=torch.int32, device=dev)            # 256 MB, written four times: pending work
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        for v in range(4):
            ballast.fill_(v)
        rc = eng.lib.msr_match_sets(eng.handle, len(rows), _P(g_off), _P(t_off), _P(terms), _P(need), _P(bb), 3, bs, _P(rb), _P(out),
                                    W + PAD, C.c_void_p(side.cuda_stream))
        assert rc == 0, eng.lib.msr_last_error(eng.handle)
    side.synchronize()                                       # the output is not read before the caller's stream is done
    assert out.cpu().numpy().view(np.uint32).tobytes() == want.tobytes()
    assert int(ballast[-1]) == 3


# ------------------------------------------------------------------------------------------------ the engine call
def test_match_sets_row_sharing_and_every_kind_of_within(corp, eng):
    c = corp
    a, b, d, l = c.mid[0], c.mid[1], c.mid[2], c.light[0]
    odd, rnd = DocSet.from_mask(c.ix, c.bases[0]), DocSet.from_mask(c.ix, c.bases[2])
    groups = [[[a], [b], [d]], [[d], [a], [b, b]], [[a], [b], [d]], [[a], [b], [d]], [[a, l], [b]], [[a]], [[a], [-1]], [[a], [c.V + 5]], [],
              [[a], [b], [d]], [[c.empty, a], [b], [d]]]
    need = [2, 2, 3, 2, 2, None, 2, 2, None, 2, 2]
    within = [None, None, None, odd, None, odd, None, None, None, rnd, None]
    ds = mt.match_sets(eng, groups, need, within=within)
    assert isinstance(ds, DeviceSets) and len(ds) == len(groups) and ds.stride == W
    q = ds.q_set.cpu().tolist()
    assert q[0] == q[1] == q[10] and q[0] != q[2] and q[0] != q[3] and q[3] != q[9]      # groups as sets, need and base decide
    assert q[6] == q[7]                                      # every id the index lacks is the same empty slot
    assert q[8] == -1 and ds.docset(5) == odd                # matching off: the base's row, or -1, and no kernel row
    assert ds.n_sets == 2 + len({q[i] for i in (0, 2, 3, 4, 6, 9)}) == 8      # the two base rows, then one row per distinct key
    assert eng.pack_within(ds, len(groups))[0] is ds.bits    # handed on unchanged to every consumer
    for i in range(len(groups)):
        bm = None if within[i] is None else within[i].mask
        want = match_mask(c.z, groups[i], need[i] or 0, bm)
        assert ds.docset(i) == DocSet.from_mask(c.ix, want), i
    # one DocSet for every query; no within at all: no base rows
    one = mt.match_sets(eng, groups[:3], need[:3], within=odd)
    assert all(one.docset(i) == DocSet.from_mask(c.ix, match_mask(c.z, groups[i], need[i], odd.mask)) for i in range(3))
    bare = mt.match_sets(eng, groups[:3], need[:3])
    assert bare.n_sets == 2 and bare.docset(2) == DocSet.from_mask(c.ix, match_mask(c.z, groups[2], 3))
    off = mt.match_sets(eng, groups[:2], [None, None])       # nothing to match: no row, no launch
    assert off.n_sets == 0 and off.q_set.cpu().tolist() == [-1, -1]
    # a DeviceSets as the base: what operators built (Conditions.sets)
    ts = eng.term_sets([[l], [], [l], []], [[], [d], [], []], within=[None, None, odd, odd])
    on = mt.match_sets(eng, [groups[0]] * 4, [2, 2, None, None], within=ts)
    m0 = match_mask(c.z, groups[0], 2)
    assert on.docset(0) == DocSet.from_mask(c.ix, m0 & term_set_mask(c.z, [l], []))
    assert on.docset(1) == DocSet.from_mask(c.ix, m0 & term_set_mask(c.z, [], [d]))
    assert on.docset(2) == ts.docset(2) and on.docset(3) == odd
    # the sets feed the existing consumers like a host-built DocSet of the same documents
    ref = [DocSet.from_mask(c.ix, match_mask(c.z, groups[i], need[i] or 0, None if within[i] is None else within[i].mask))
           for i in range(len(groups))]
    terms = [[a, b, d, 0]] * len(groups)
    for got, want in zip(eng.bm25_topk(terms, k=100, within=ds), eng.bm25_topk(terms, k=100, within=ref)):
        assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
    # refusals of the host
    with pytest.raises(ValueError, match="MSR_MATCH_MAX_GROUPS"):
        mt.match_sets(eng, [[[a]] * 65], [1])
    with pytest.raises(ValueError):
        mt.match_sets(eng, groups[:2], [1])
    with pytest.raises(ValueError):
        mt.match_sets(eng, groups[:2], [1, 1], within=ts)
    assert mt.match_sets(eng, [[[a]] * 65], [None]).n_sets == 0              # (matching off: the slots are not looked at)


# ------------------------------------------------------------------------------------------------ the facades
QUERY = "mensa morgenstelle öffnungszeiten"


def _slot_count(c, rows, slot_terms):
    """Per result row: how many of the slots its document fills, from the postings."""
    docs = [set(np.nonzero(group_mask(c.z, g))[0].tolist()) for g in slot_terms]
    return [sum(c.pos[row["doc_id"]] in d for d in docs) for row in rows]


@pytest.mark.parametrize("mode", ["lexical", "hybrid"])
def test_retriever_search_all_two_and_a_share(corp, eng, mode):
    c = corp
    r = Retriever(indexer=eng)
    e0 = c.qv[0]
    slots = [[c.named[w]] for w in ("mensa", "morgenstelle", "öffnungszeiten")]
    plain = r.search(QUERY, query_embedding=e0, mode=mode)
    assert type(plain) is list and plain
    sizes = []
    for value, need in (("all", 3), (2, 2), ("75%", 2), (-1, 2), (1, 1)):
        got = r.search(QUERY, query_embedding=e0, mode=mode, match=value)
        assert isinstance(got, Results) and got
        assert got.match == {"slots": [["mensa"], ["morgenstelle"], ["öffnungszeiten"]], "need": need}    # (no city slot)
        assert min(_slot_count(c, got, slots)) >= need, value
        ref = DocSet.from_mask(c.ix, match_mask(c.z, slots, need))
        assert got == r.search(QUERY, query_embedding=e0, mode=mode, within=ref), value
        sizes.append(len(ref))
    assert 0 < sizes[0] < sizes[1] == sizes[2] == sizes[3] < sizes[4] < N_DOCS
    # match="any" is the call without the keyword, row for row, and the same plain list
    for any_ in ("any", None):
        same = r.search(QUERY, query_embedding=e0, mode=mode, match=any_)
        assert type(same) is list and same == plain
    # a word the vocabulary lacks is a slot that nobody fills -- in both stages
    none = r.search(QUERY + " xqzw", query_embedding=e0, mode=mode, match="all")
    assert none == [] and none.match["need"] == 4 and none.match["slots"][-1] == ["xqzw"]
    assert r.search(QUERY + " xqzw", query_embedding=e0, mode=mode, match=3) == \
        r.search(QUERY + " xqzw", query_embedding=e0, mode=mode, within=DocSet.from_mask(c.ix, match_mask(c.z, slots, 3)))
    with pytest.raises(ValueError, match="match must be"):
        r.search(QUERY, query_embedding=e0, mode=mode, match="most")


def test_match_with_the_other_options(corp, eng):
    c = corp
    r = Retriever(indexer=eng)
    e0 = c.qv[0]
    M, MA, MO, OE = (c.named[w] for w in NAMED)
    three = [[M], [MO], [OE]]
    # within= and operators: the count is taken inside what they built
    site = DocSet.from_sites(c.ix, ["uni-tuebingen.de"])
    got = r.search(QUERY, query_embedding=e0, match="all", within=site)
    assert got and got == r.search(QUERY, query_embedding=e0, within=site & DocSet.from_mask(c.ix, match_mask(c.z, three, 3)))
    ops = r.search(f"mensa +morgenstelle öffnungszeiten -{_word(c.mid[30])}", query_embedding=e0, operators=True, match=2)
    want = term_set_mask(c.z, [MO], [c.mid[30]]) & match_mask(c.z, three, 2)
    assert ops and ops == r.search(QUERY, query_embedding=e0, within=DocSet.from_mask(c.ix, want))
    # wildcards: a pattern's expansions are ONE slot
    wild = r.search("mensa* morgenstelle", query_embedding=e0, wildcards=True, match="all")
    assert wild.match == {"slots": [["morgenstelle"], ["mensa", "mensaria"]], "need": 2} or \
        wild.match == {"slots": [["morgenstelle"], ["mensaria", "mensa"]], "need": 2}
    ref = DocSet.from_mask(c.ix, match_mask(c.z, [[MO], [M, MA]], 2))
    assert wild and wild == r.search("mensa* morgenstelle", query_embedding=e0, wildcards=True, within=ref)
    assert len(ref) > int(match_mask(c.z, [[MO], [M]], 2).sum())
    assert list(wild.expansions) == ["mensa*"]
    # fuzzy runs first: the corrected word is the slot
    typo = r.search("mensx morgenstelle", query_embedding=e0, fuzzy=True, match="all")
    assert typo.corrections == {"mensx": "mensa"} and typo.match == {"slots": [["mensa"], ["morgenstelle"]], "need": 2}
    ref = DocSet.from_mask(c.ix, match_mask(c.z, [[M], [MO]], 2))
    assert typo and typo == r.search("mensx morgenstelle", query_embedding=e0, fuzzy=True, within=ref)
    assert r.search("mensx morgenstelle", query_embedding=e0, match="all") == []
    # facets count inside the matched set: "how many pages hold all my words"
    for value, need in (("all", 3), (2, 2)):
        f = r.search(QUERY, query_embedding=e0, facets=True, match=value)
        assert f.hits == int(match_mask(c.z, three, need).sum()) and sum(x["count"] for x in f.facets) == f.hits
    assert r.search(QUERY, query_embedding=e0, facets=True).hits == int(match_mask(c.z, three, 1).sum())
    # a typed city is no slot either; a query of the city alone keeps it (the fallback)
    assert r.search(QUERY + " tübingen", query_embedding=e0, match="all").match["need"] == 3
    assert r.search("tübingen", query_embedding=e0, match="all").match == {"slots": [["tübingen"]], "need": 1}


def test_batches_final_lists_and_the_bm25_facade(corp, eng):
    c = corp
    r = Retriever(indexer=eng)
    M, MA, MO, OE = (c.named[w] for w in NAMED)
    qs = [QUERY, "mensa", "mensaria morgenstelle", QUERY, "xqzw"]
    got = r.search_batch(qs, query_embeddings=c.qv[:5], match="all")
    for q in range(5):
        assert got[q] == r.search(qs[q], query_embedding=c.qv[q], match="all"), q
        assert got[q].match == r.search(qs[q], query_embedding=c.qv[q], match="all").match
    assert [g.match["need"] for g in got] == [3, 1, 2, 3, 2] and got[4] == [] and got[0] and got[2]      # ("xqzw tübingen": 2)
    lines = r.batch_search(list(zip("12345", qs)), query_embeddings=c.qv[:5], match="all")
    assert lines.match == [g.match for g in got]
    assert [e["url"] for e in lines if e["query_num"] == "3"][:100] == [d["url"] for d in got[2]]
    assert r.batch_search(list(zip("12", qs[:2])), query_embeddings=c.qv[:2]).match is None
    # term ids in: the lists are the slots; the dict form says what was required
    ids = [[M, MO, OE, 0], [M, M, MA], [MO, -1], []]
    info = {"value": 2}
    out = r.final_lists(ids, c.qv[:4], 1000, match=info, chunk=3)
    assert info["need"] == [2, 2, 2, None] and info["slots"] == [[[M], [MO], [OE]], [[M], [MA]], [[MO], [-1]], []]
    ref = [DocSet.from_mask(c.ix, match_mask(c.z, g, n or 0)) for g, n in zip(info["slots"], info["need"])]
    want = r.final_lists(ids, c.qv[:4], 1000, within=ref)
    for a, b in zip(out, want):
        assert a.tobytes() == b.tobytes()
    assert int(out[3][0]) > 0 and int(out[3][2]) == 0
    for a, b in zip(r.final_lists(ids, c.qv[:4], 1000, match=2, mode="hybrid", with_source=True),
                    r.final_lists(ids, c.qv[:4], 1000, within=ref, mode="hybrid", with_source=True)):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(r.final_lists(ids, c.qv[:4], 1000, match="any"), r.final_lists(ids, c.qv[:4], 1000)):
        assert a.tobytes() == b.tobytes()
    chunks = list(r.final_list_chunks(ids, c.qv[:4], 1000, match=2, chunk=2))
    assert len(chunks) == 2 and np.concatenate([ch[4] for ch in chunks]).tolist() == out[3].tolist()
    with pytest.raises(ValueError, match="slots"):
        r.final_lists([list(c.mid[:40]) + list(c.light[:30])], c.qv[:1], 1000, match="all")
    # the BM25 facade: its query is taken as it is
    bm = r.bm25.search(QUERY, top_k=50, match="all")
    assert bm and bm.match["need"] == 3
    assert bm == r.bm25.search(QUERY, top_k=50, within=DocSet.from_mask(c.ix, match_mask(c.z, [[M], [MO], [OE]], 3)))
    assert type(r.bm25.search(QUERY, top_k=50)) is list and r.bm25.search(QUERY, top_k=50, match="any") == r.bm25.search(QUERY, top_k=50)
    assert r.bm25.search(QUERY + " xqzw", match="all") == []
    both = r.bm25.search(f"mensa +morgenstelle öffnungszeiten", top_k=50, operators=True, match=2)
    assert both == r.bm25.search(QUERY, top_k=50, within=DocSet.from_mask(
        c.ix, term_set_mask(c.z, [MO], []) & match_mask(c.z, [[M], [MO], [OE]], 2)))


def test_http_search_with_match(corp, eng):
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from msretr.server import create_app
    c = corp
    r = Retriever(indexer=eng)
    client = TestClient(create_app(r))
    body = {"query": QUERY, "top_k": 1000, "query_id": "q1", "query_embedding": c.qv[0].tolist()}
    plain = client.post("/api/search", json=body)
    assert plain.status_code == 200 and "match" not in plain.json()
    for value in ("all", 2, "75%"):
        res = client.post("/api/search", json=dict(body, match=value))
        want = r.search(QUERY, top_k=1000, query_embedding=c.qv[0], query_id="q1", match=value)
        assert res.status_code == 200 and res.json()["documents"] == want and want
        assert res.json()["match"] == want.match
    assert client.post("/api/search", json=dict(body, match="any")).json() == plain.json()
    assert client.post("/api/search", json=dict(body, match="most")).status_code == 400
    assert client.post("/api/search", json=dict(body, match=0)).status_code == 400
